"""The `ddpminv` and `cyclediff` inverters on the engine: plugin + simple editor against tests/golden/ddpminv_sd.npz (tests/ddpminv_ref.py over
the SD-width oracle UNet in float64, 16 x 16 latents, S = 5: one step skipped, four run, t = 0 with sigma = 0 among them), the time-parallel
inversion against the per-step one, prompt-to-prompt and MasaCtrl through the per-step backward pass, the skip, the batched DdpmLoop and the
command line.  The forward noise is the fixture's, through `forward_noise` (a ROCm generator's stream is not the CPU generator's).

Bounds.  fp32 pipeline: the project's 1e-3 relative L2 on noise predictions, inversion latents and both edited rows.  fp16 pipeline: the
project's 3e-2 on the edited rows and on the inversion's noise predictions.  The noise maps get no tolerance of their own: a map amplifies the
UNet's error by |c_eps| / sigma (about 20 at t = 200 for S = 5), exactly, dz = -c_eps d_eps / sigma.  So the run's maps are compared with the
float64 step evaluated on the run's OWN noise predictions and the fixture's noised latents, and must agree at fp32 rounding:
|dz| <= (3 S + 8) 2^-24 M / sigma per element, M = max|x_{t-1}| + (sqrt(abar_prev) / sqrt(abar_t)) (max|x_t| + sqrt(1 - abar_t) max|eps|)
+ c_dir max|eps| the sum of the magnitudes that enter z -- three roundings per link of the noising chain (at most S links) for each of x_t and
x_{t-1}, and eight for the step itself (two coefficients' worth of rounding included).

Measured on MI355X (this file's own printouts): see DESIGN.md, "DDPM inversion"."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import ddpminv_ref as dr
from tests import edict_ref as er

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
SRC, TGT = "a cat sitting next to a mirror", "a tiger sitting next to a mirror"
L, S = er.SD_L, 5
MODES = ("ddpminv", "cyclediff")


def rel(a, b):
    a, b = (v.detach().double().cpu() if torch.is_tensor(v) else torch.as_tensor(np.asarray(v)).double() for v in (a, b))
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def case():
    z0, ctx_s, ctx_t = er.sd_case_inputs()
    g = np.load(ROOT / "tests" / "golden" / "ddpminv_sd.npz")
    assert int(g["S"]) == S and dr.bwd_skip(S) == 1
    np.testing.assert_array_equal(np.concatenate([z0.ravel()[:4], ctx_s.ravel()[:4], ctx_t.ravel()[:4], g["noise"].ravel()[:4]]), g["probe"])
    f = lambda v: torch.from_numpy(v).float().cuda()
    return dict(z0=f(z0), ctx={SRC: f(ctx_s), TGT: f(ctx_t)}, noise=f(g["noise"]), g=g)


@pytest.fixture(scope="module")
def pipes():
    """(variant, max_img) -> pipeline, built on first use, one each for the whole module"""
    import modules
    made = {}

    def get(variant, max_img=3):
        if (variant, max_img) not in made:
            made[variant, max_img] = modules.load_diffusion_model("sd15", "cuda", variant=variant, latent_size=L, max_img=max_img)[0]
        return made[variant, max_img]
    yield get
    for p in made.values():
        p.engine.close()


def _inverter(p, case, name="ddpminv", **kw):
    """the inverter fed with the case's latent, contexts and noise directly (the VAE and the text encoder are tested elsewhere)"""
    import modules
    inv = modules.load_inverter(name, model=p, scheduler="ddim", num_inference_steps=S, **kw)
    inv.encode = lambda image: image.to("cuda").float()
    inv.create_context = lambda prompt, negative_prompt="": case["ctx"][prompt]
    inv.forward_noise = case["noise"]
    return inv


def _count_unet(p):
    """counts the engine's UNet calls (rows per call) until `restore()`"""
    calls, orig = [], p.engine.unet

    def counted(latent, t, ctx, ctrl=None, out=None):
        calls.append(ctx.shape[0])
        return orig(latent, t, ctx, ctrl, out=out)
    p.engine.unet = counted

    def restore():
        del p.engine.unet
    return calls, restore


def _maps_follow_their_noise(res, g, tag):
    """the run's noise maps against the float64 step on the run's own noise predictions (this file's docstring); returns the worst |dz| / bound"""
    xts, worst = g[f"{tag}/xts"], 0.0
    assert not res["variance_noises"][0].any()                                       # t = 0: zeroed
    for i, t in enumerate(dr.timesteps(S)):
        if i == 0:
            continue
        idx, c = S - 1 - i, dr.step_coefficients(S, t)
        eps = res["noise_preds"][i].double().cpu().numpy()
        z = dr.inverse_step(xts[idx], xts[idx + 1], eps, c)[0]
        m = np.abs(xts[idx + 1]).max() + c[2] / c[1] * (np.abs(xts[idx]).max() + c[0] * np.abs(eps).max()) + c[3] * np.abs(eps).max()
        bound = (3 * S + 8) * 2.0 ** -24 * m / c[4]
        worst = max(worst, float(np.abs(res["variance_noises"][i].double().cpu().numpy() - z).max() / bound))
    return worst


def _edit_vs_oracle(p, case, tag, variant):
    """invert + simple edit; returns (noise prediction error, inversion latent error, source error, target error, worst map deviation / bound)"""
    import modules
    g = case["g"]
    inv = _inverter(p, case, tag)
    assert inv.markovian_forward == (tag == "cyclediff") and (inv.guidance_scale_fwd, inv.guidance_scale_bwd, inv.skip_steps) == (3.5, 9, 0.36)
    res = inv.invert(case["z0"], prompt=SRC, context=case["ctx"][SRC], guidance_scale_fwd=1)          # what the simple editor passes
    assert {"latents", "noise_preds", "etas", "variance_noises", "context"} <= set(res)
    assert len(res["latents"]) == S + 1 and len(res["noise_preds"]) == len(res["variance_noises"]) == S and res["etas"] == [1.0] * S
    assert all(torch.isfinite(v).all() for v in res["latents"] + res["variance_noises"])           # the sigma == 0 step included
    e_eps = rel(torch.stack(res["noise_preds"]), g[f"{tag}/noise_preds"])
    e_lat = rel(torch.stack(res["latents"]), g[f"{tag}/latents"])
    worst = _maps_follow_their_noise(res, g, tag)
    edit = modules.load_editor("simple", inverter=inv).edit(case["z0"], SRC, TGT)
    assert set(edit) == {"image_inv", "image", "latent_inv", "latent"} and edit["image"].shape == (1, 3, 8 * L, 8 * L)
    e_s, e_t = rel(edit["latent_inv"], g[f"{tag}/edit"][0:1]), rel(edit["latent"], g[f"{tag}/edit"][1:2])
    print(f"{tag} + simple vs oracle ({variant}): noise predictions rel L2 {e_eps:.3e}, inversion latents {e_lat:.3e}, edited latents source {e_s:.3e}, "
          f"target {e_t:.3e}; noise maps vs their own noise: worst |dz| / bound {worst:.3f}")
    return e_eps, e_lat, e_s, e_t, worst


@pytest.mark.parametrize("tag", MODES)
def test_plugin_simple_vs_oracle_fp32(pipes, case, tag):
    e_eps, e_lat, e_s, e_t, worst = _edit_vs_oracle(pipes("fp32"), case, tag, "fp32")
    assert e_eps < 1e-3 and e_lat < 1e-3 and e_s < 1e-3 and e_t < 1e-3
    assert worst <= 1.0


@pytest.mark.parametrize("tag", MODES)
def test_plugin_simple_vs_oracle_fp16(pipes, case, tag):
    e_eps, _, e_s, e_t, worst = _edit_vs_oracle(pipes("fp16"), case, tag, "fp16")
    assert e_eps < 3e-2 and e_s < 3e-2 and e_t < 3e-2
    assert worst <= 1.0                                                              # the step kernels are fp32 whatever the UNet's precision


def test_time_parallel_against_per_step(pipes, case):
    """on a max_img = 1 engine (4 rows per call) the guided inversion of 5 steps is chunks of 2, 2 and 1 steps: 3 UNet calls against 5"""
    g, p = case["g"], pipes("fp32", 1)
    assert p.engine.max_unet_batch == 4
    inv = _inverter(p, case)
    calls, restore = _count_unet(p)
    try:
        fast = inv.invert(case["z0"], context=case["ctx"][SRC])
        n_fast = list(calls)
        calls.clear()
        inv.force_per_step = True
        slow = inv.invert(case["z0"], context=case["ctx"][SRC])
        n_slow = list(calls)
        calls.clear()
        ed_slow = inv.sample(slow, context=[case["ctx"][SRC], case["ctx"][TGT]])["latent"]
        n_bwd_slow = list(calls)
        calls.clear()
        inv.force_per_step = False
        ed_fast = inv.sample(fast, context=[case["ctx"][SRC], case["ctx"][TGT]])["latent"]
        n_bwd_fast = list(calls)
    finally:
        restore()
    assert n_fast == [4, 4, 2] and n_slow == [2] * S
    assert n_bwd_fast == n_bwd_slow == [4] * (S - 1)                                 # one step skipped
    for name, key in (("noise_preds", "noise_preds"), ("latents", "latents"), ("variance_noises", "zs")):
        a, b, want = torch.stack(fast[name]), torch.stack(slow[name]), g[f"ddpminv/g35/{key}"]
        ea, eb, ab = rel(a, want), rel(b, want), rel(a, b)
        print(f"{name}: time-parallel vs oracle {ea:.3e}, per-step vs oracle {eb:.3e}, one against the other {ab:.3e}")
        if name != "variance_noises":                                               # (the maps: held to their own noise below)
            assert ea < 1e-3 and eb < 1e-3 and ab < 1e-3
    assert _maps_follow_their_noise(fast, g, "ddpminv") <= 1.0 and _maps_follow_their_noise(slow, g, "ddpminv") <= 1.0
    ea, eb, ab = rel(ed_fast, g["ddpminv/g35/edit"]), rel(ed_slow, g["ddpminv/g35/edit"]), rel(ed_fast, ed_slow)
    print(f"edited rows after the guided inversion: fused path vs oracle {ea:.3e}, per-step path {eb:.3e}, one against the other {ab:.3e}")
    assert ea < 1e-3 and eb < 1e-3 and ab < 1e-3


def test_attention_editors_run_the_per_step_path(pipes, case):
    import modules
    p = pipes("fp32")
    inv = _inverter(p, case)
    simple = modules.load_editor("simple", inverter=inv).edit(case["z0"], SRC, TGT)
    ptp_cfg = dict(is_replace_controller=False, prompts=[SRC, TGT], cross_replace_steps={"default_": .4}, self_replace_steps=0.6,
                   equilizer_params={"words": ("tiger",), "values": (2,)})
    for editor, cfg in (("ptp", ptp_cfg), ("masactrl", None)):
        steps, orig = [], inv.predict_step_backward

        def counted(latent, t, *a, _o=orig, **k):
            steps.append(int(t))
            return _o(latent, t, *a, **k)
        inv.predict_step_backward = counted
        try:
            ed = modules.load_editor(editor, inverter=inv) if cfg else modules.load_editor(editor, inverter=inv, step=1, layer=4)
            res = ed.edit(case["z0"], SRC, TGT, cfg={**cfg} if cfg else None)
        finally:
            del inv.predict_step_backward
        assert steps == [600, 400, 200, 0] and p.unet.attn_ctrl is None                # the steps behind the skip, hooked one by one
        assert torch.isfinite(res["latent"]).all() and torch.isfinite(res["latent_inv"]).all()
        moved = rel(res["latent"], simple["latent"])
        print(f"ddpminv + {editor}: target differs from simple by {moved:.3e}, source row by {rel(res['latent_inv'], simple['latent_inv']):.3e}")
        assert moved > 1e-3                                                            # the attention edit changes the target row
    with pytest.raises(NotImplementedError, match="pnp editor"):
        modules.load_editor("pnp", inverter=inv)


def test_hooked_backward_path_matches_the_fused_one(pipes, case):
    """a controller that only counts: the per-step backward path (cfg_combine per row + ddim_eta_step) against the fused launch"""
    from modules.editing.controller import ControllerBase
    inv = _inverter(pipes("fp32"), case)
    res = inv.invert(case["z0"], context=case["ctx"][SRC], guidance_scale_fwd=1)
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
    with inv.use_controller(rec):
        slow = inv.sample(res, context=contexts)["latent"]
    assert (rec.begun, rec.ended) == (S - 1, S - 1)
    e = rel(fast, slow)
    print(f"ddpminv: fused vs hooked backward path rel L2 {e:.3e}; vs oracle {rel(slow, case['g']['ddpminv/edit']):.3e}")
    assert e < 1e-3 and rel(slow, case["g"]["ddpminv/edit"]) < 1e-3
    one = inv.sample(res, context=case["ctx"][TGT])["latent"]                        # a single prompt runs under guidance_scale_bwd
    assert one.shape == (1, 4, L, L) and rel(one, fast[1:2]) < 1e-3


@pytest.mark.parametrize("skip_steps,skipped", [(0.1, 0), (0.36, 1), (0.5, 2)])
def test_skip_steps(pipes, case, skip_steps, skipped):
    """int(skip_steps * 5) = 0, 1, 2 skipped steps; 0 skips nothing (the reference's [:-0] would empty the trajectory)"""
    p = pipes("fp32")
    inv = _inverter(p, case, skip_steps=skip_steps)
    assert inv.get_bwd_skip() == skipped
    res = inv.invert(case["z0"], context=case["ctx"][SRC], guidance_scale_fwd=1)
    cut = inv.skip_inv_result(res)
    assert len(cut["latents"]) == S + 1 - skipped and len(cut["variance_noises"]) == len(cut["noise_preds"]) == len(cut["etas"]) == S - skipped
    assert len(res["latents"]) == S + 1                                              # (the result itself is not cut)
    calls, restore = _count_unet(p)
    try:
        out = inv.sample(res, context=[case["ctx"][SRC], case["ctx"][TGT]])["latent"]
    finally:
        restore()
    assert calls == [4] * (S - skipped) and torch.isfinite(out).all()
    ref = dr.DdpmInvRef(None, S, skip_steps=skip_steps)
    assert dr.bwd_skip(S, skip_steps) == skipped and ref.t_bwd[skipped:].tolist() == [800, 600, 400, 200, 0][skipped:]
    if skipped == 1:
        assert rel(out, case["g"]["ddpminv/edit"]) < 1e-3


def test_ddpm_loop_batch_of_three(pipes, case):
    """DdpmLoop with B = 3 (the case's image, and two scaled copies with other noise) against three B = 1 runs"""
    from etainv.flops import ddpm_unet_rows
    from etainv.pipeline import DdpmLoop
    p = pipes("fp32")
    z0 = torch.cat([case["z0"], 0.9 * case["z0"].flip(-1), 1.1 * case["z0"].flip(-2)])
    noise = torch.cat([case["noise"], case["noise"].flip(0), case["noise"].flip(-1)], dim=1)
    ctx = [torch.stack([case["ctx"][k]] * 3) for k in (SRC, TGT)]
    loop = DdpmLoop(p.engine, S=S)
    inv = loop.invert(z0, ctx[0], noise, 1.0)
    assert loop.unet_calls == 2 and inv["xts"].shape == (S + 1, 3, 4, L, L)           # 15 rows through a 12-row engine
    out = loop.sample(inv, ctx)
    assert out.shape == (6, 4, L, L) and loop.rows_executed == ddpm_unet_rows(S, 1, 3, 2, g_fwd=1) == loop.expected_rows(3, 2, 1.0) == 63
    for b in range(3):
        one = DdpmLoop(p.engine, S=S)
        inv1 = one.invert(z0[b:b + 1], ctx[0][b:b + 1], noise[:, b:b + 1].contiguous(), 1.0)
        out1 = one.sample(inv1, [c[b:b + 1] for c in ctx])
        assert one.rows_executed == ddpm_unet_rows(S, 1, 1, 2, g_fwd=1) == 21
        assert torch.equal(inv1["xts"][:, 0], inv["xts"][:, b])                      # the noising does not depend on the batch
        e_eps, e_s, e_t = rel(inv["noise_preds"][:, b], inv1["noise_preds"][:, 0]), rel(out[b], out1[0]), rel(out[3 + b], out1[1])
        print(f"DdpmLoop image {b}: B = 3 vs B = 1 noise predictions {e_eps:.3e}, source row {e_s:.3e}, target row {e_t:.3e}")
        assert e_eps < 1e-3 and e_s < 1e-3 and e_t < 1e-3
        if b == 0:
            assert rel(out1, case["g"]["ddpminv/edit"]) < 1e-3
    guided = DdpmLoop(p.engine, S=S)
    guided.invert(z0[:1], ctx[0][:1], noise[:, :1].contiguous())
    assert guided.unet_calls == 1 and guided.rows_executed == 10                     # 5 steps x [u, c] in one 12-row call


def test_edit_image_cli_ddpminv(tmp_path):
    from PIL import Image
    src = tmp_path / "in.png"
    Image.fromarray((np.random.default_rng(0).random((96, 96, 3)) * 255).astype(np.uint8)).save(src)
    out = tmp_path / "out.png"
    r = subprocess.run([sys.executable, str(ROOT / "eta-inversion_amd" / "edit_image.py"), "--input", str(src), "--source_prompt", SRC,
                        "--target_prompt", TGT, "--output", str(out), "--inv_method", "ddpminv", "--edit_method", "simple", "--steps", "3",
                        "--prec", "fp16"], capture_output=True, text=True, timeout=900,
                       env={**__import__("os").environ, "PYTHONPATH": str(ROOT / "eta-inversion_amd")})
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Saved result to" in r.stdout and "Took" in r.stdout
    assert out.exists() and (tmp_path / "out_inv.png").exists()
    assert Image.open(out).size == (512, 512)
