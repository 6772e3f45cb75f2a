"""The `regdiffinv` inverter on the engine: plugin + simple editor against tests/golden/regdiff_sd.npz (tests/regdiff_ref.py over the
SD-width oracle UNet in float64, 16 x 16 latents, S = 3), fast path == per-step path, the batched loop, prompt-to-prompt through the
per-step backward pass, and the command line.

Bounds.  fp32 pipeline: the project's 1e-3 relative L2.  fp16 pipeline: the run with the regularisation off (num_reg_steps = 0: the same
fused launch, passing the noise through) holds the project's 5e-3; the regularised run may be at most 3 x that run's measured error -- the
regulariser is an iteration on the noise the 16-bit UNet predicted, and the 3 is room for what it does to that noise's error.

Measured on MI355X (this file's own printouts): see DESIGN.md, "Regularised DDIM inversion"."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import edict_ref as er
from tests import regdiff_ref as rr

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
    g = np.load(ROOT / "tests" / "golden" / "regdiff_sd.npz")
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


@pytest.fixture(params=["fp32", "fp16"])
def pipe(request, pipes):
    return request.param, pipes(request.param)


def _inverter(p, case, **kw):
    """the inverter fed with the case's latent and contexts directly (the VAE and the text encoder are tested elsewhere)"""
    import modules
    inv = modules.load_inverter("regdiffinv", model=p, scheduler="ddim", num_inference_steps=S, **kw)
    inv.encode = lambda image: image.to("cuda").float()
    inv.create_context = lambda prompt, negative_prompt="": case["ctx"][prompt]
    return inv


def test_plugin_simple_vs_oracle(pipe, case):
    import modules
    variant, p = pipe
    g = case["g"]
    inv = _inverter(p, case)
    res = inv.invert(case["z0"], prompt=SRC, context=case["ctx"][SRC])
    assert {"latents", "noise_preds", "zT_inv", "context"} <= set(res) and len(res["latents"]) == S + 1 and len(res["noise_preds"]) == S
    assert inv._loop.rows_executed == 2 * 1 * S
    lat, eps = torch.stack(res["latents"]), torch.stack(res["noise_preds"])
    e_inv, e_eps = rel(lat, g["inv_latents"]), rel(eps, g["noise_preds"])
    off = _inverter(p, case, num_reg_steps=0)
    e_off = rel(torch.stack(off.invert(case["z0"], context=case["ctx"][SRC])["latents"]), g["inv_latents_noreg"])
    moved = rel(g["inv_latents"], g["inv_latents_noreg"])
    print(f"regdiffinv vs oracle ({variant}): inversion rel L2 {e_inv:.3e}, regularised noises {e_eps:.3e}; regularisation off {e_off:.3e} "
          f"(ratio {e_inv / e_off:.2f}); the regularisation moves the trajectory by {moved:.3e}")
    if variant == "fp32":
        assert e_inv < 1e-3 and e_eps < 1e-3 and e_off < 1e-3
    else:
        assert e_off < 5e-3 and e_inv <= 3 * e_off and e_eps <= 3 * e_off
    # each latent is the DDIM inverse step of the one before it on the returned (regularised) noise
    lp = inv._loop
    for j, t in enumerate(lp.t_fwd):
        want = rr.ddim_inverse_step(lat[j].double().cpu().numpy(), eps[j].double().cpu().numpy(), lp._alpha(int(t) - lp.delta), lp._alpha(int(t)))
        assert rel(lat[j + 1], want) < 1e-5
    edit = modules.load_editor("simple", inverter=inv).edit(case["z0"], SRC, TGT)
    assert set(edit) == {"image_inv", "image", "latent_inv", "latent"} and edit["image"].shape == (1, 3, 8 * L, 8 * L)
    e_s, e_t = rel(edit["latent_inv"], g["edit"][0:1]), rel(edit["latent"], g["edit"][1:2])
    print(f"regdiffinv + simple vs oracle ({variant}): edited latents rel L2 source {e_s:.3e}, target {e_t:.3e}")
    b_edit = 1e-3 if variant == "fp32" else 3e-2          # fp16: what test_diffinv_plugin_vs_oracle / test_edict_gpu hold on edited latents
    assert e_s < b_edit and e_t < b_edit


def test_fast_path_equals_per_step_path(pipe, case):
    """the batched loop (one fused launch per step) vs predict_step_forward (UNet, CFG kernel, regulariser alone, scheduler step) with a
    controller watching: hooks called once per step, results within the fp32 bound"""
    from modules.editing.controller import ControllerBase
    variant, p = pipe
    inv = _inverter(p, case)
    ctx = case["ctx"][SRC]
    fast = inv.invert(case["z0"], context=ctx)
    rows = inv._loop.rows_executed

    class Recording(ControllerBase):
        begun = ended = 0

        def begin_step(self, latent, *a, **k):
            self.begun += 1
            return latent

        def end_step(self, latent, noise_pred=None, t=None):
            assert noise_pred is not None and t is not None
            self.ended += 1
            return latent
    rec = Recording()
    with inv.use_controller(rec):
        slow = inv.invert(case["z0"], context=ctx)
    assert (rec.begun, rec.ended) == (S, S) and inv._loop.rows_executed == rows       # the loop did not run
    inv.force_per_step = True
    forced = inv.invert(case["z0"], context=ctx)
    inv.force_per_step = False
    e_lat = rel(torch.stack(slow["latents"]), torch.stack(fast["latents"]))
    e_eps = rel(torch.stack(slow["noise_preds"]), torch.stack(fast["noise_preds"]))
    print(f"per-step vs fast path ({variant}): latents rel L2 {e_lat:.3e}, regularised noises {e_eps:.3e}")
    assert e_lat < 1e-3 and e_eps < 1e-3
    assert rel(torch.stack(forced["latents"]), torch.stack(slow["latents"])) < 1e-5    # the same calls, with and without a controller
    # regularize_noise_pred with a generator seeded like predict_step_forward's gives the step's regularisation
    plain = _inverter(p, case, num_reg_steps=0).invert(case["z0"], context=ctx)["noise_preds"][0]
    again = inv.regularize_noise_pred(plain, generator=torch.Generator().manual_seed(0))
    assert rel(again, fast["noise_preds"][0]) < 1e-5


def test_loop_batch_of_three_equals_single_runs(pipes, case):
    """EtaLoop with the regulariser at B = 3 vs three B = 1 runs, fp32, at the inversion bound of tests/test_batch_gpu.py (2e-3)"""
    from etainv.pipeline import EtaLoop, NoiseRegularizer
    p = pipes("fp32")
    gen = torch.Generator().manual_seed(5)
    z0 = torch.cat([case["z0"].cpu(), 0.8 * torch.randn(2, 4, L, L, generator=gen)]).cuda()
    c = case["ctx"][SRC]
    ctx = torch.stack([c, c + 0.05 * torch.randn(c.shape, generator=gen).cuda(), c.flip(1)]).contiguous()
    mk = lambda: EtaLoop(p.engine, S=S, guidance_scale_fwd=(2.0, 1.0), use_mask=False, regularizer=NoiseRegularizer(L))
    loop = mk()
    inv = loop.invert(z0, ctx)
    assert inv["latents"].shape == (S + 1, 3, 4, L, L) and inv["noise_preds"].shape == (S, 3, 4, L, L)
    assert loop.rows_executed == 2 * 3 * S
    for i in range(3):
        one = mk()
        inv1 = one.invert(z0[i:i + 1], ctx[i:i + 1])
        e_lat, e_eps = rel(inv["latents"][:, i:i + 1], inv1["latents"]), rel(inv["noise_preds"][:, i:i + 1], inv1["noise_preds"])
        print(f"B = 3 vs B = 1, image {i}: inversion rel L2 {e_lat:.3e}, regularised noises {e_eps:.3e}")
        assert e_lat < 2e-3 and e_eps < 2e-3
        assert one.rows_executed == 2 * S


def test_ptp_without_blend_runs_the_per_step_backward_pass(pipe, case):
    import modules
    variant, p = pipe
    inv = _inverter(p, case)
    calls = []
    orig = inv.predict_step_backward

    def counted(latent, t, *a, **k):
        calls.append(int(t))
        return orig(latent, t, *a, **k)
    inv.predict_step_backward = counted
    cfg = dict(is_replace_controller=False, prompts=[SRC, TGT], cross_replace_steps={"default_": .4}, self_replace_steps=0.6,
               equilizer_params={"words": ("tiger",), "values": (2,)})
    res = modules.load_editor("ptp", inverter=inv).edit(case["z0"], SRC, TGT, cfg={**cfg})
    assert len(calls) == S and p.unet.attn_ctrl is None
    calls.clear()
    simple = modules.load_editor("simple", inverter=inv).edit(case["z0"], SRC, TGT)
    assert torch.isfinite(res["latent"]).all() and torch.isfinite(res["latent_inv"]).all()
    assert rel(res["latent"], simple["latent"]) > 1e-3                                 # the attention edit changes the target row


def test_edit_image_cli_regdiffinv(tmp_path):
    from PIL import Image
    src = tmp_path / "in.png"
    Image.fromarray((np.random.default_rng(0).random((96, 96, 3)) * 255).astype(np.uint8)).save(src)
    out = tmp_path / "out.png"
    r = subprocess.run([sys.executable, str(ROOT / "eta-inversion_amd" / "edit_image.py"), "--input", str(src), "--source_prompt", SRC,
                        "--target_prompt", TGT, "--output", str(out), "--inv_method", "regdiffinv", "--edit_method", "simple", "--steps", "3",
                        "--prec", "fp16"], capture_output=True, text=True, timeout=900,
                       env={**__import__("os").environ, "PYTHONPATH": str(ROOT / "eta-inversion_amd")})
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Saved result to" in r.stdout and "Took" in r.stdout
    assert out.exists() and (tmp_path / "out_inv.png").exists()
    assert Image.open(out).size == (512, 512)
