"""The `edict` inverter on the engine: plugin + simple editor against tests/golden/edict_sd.npz (tests/edict_ref.py over the SD-width oracle
UNet, 16 x 16 latents, S = 3), the round trip that is EDICT's point, fast path == per-step path, the batched loop, prompt-to-prompt through
EdictController, and the command line.

Measured on MI355X (this file's own printouts): see DESIGN.md, "EDICT"."""
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
    g = np.load(ROOT / "tests" / "golden" / "edict_sd.npz")
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


def _inverter(p, case, name="edict", **kw):
    """the inverter fed with the case's latent and contexts directly (the VAE and the text encoder are tested elsewhere)"""
    import modules
    inv = modules.load_inverter(name, model=p, scheduler="ddim", num_inference_steps=S, **kw)
    latent = lambda image: image.to("cuda").float()
    inv.encode = (lambda image: [latent(image).clone(), latent(image).clone()]) if name == "edict" else latent
    inv.create_context = lambda prompt, negative_prompt="": case["ctx"][prompt]
    return inv


def test_plugin_simple_vs_oracle(pipe, case):
    """fp32: the project's fp32 tolerance, 1e-3 relative L2.  fp16: 5e-3 on the inversion and 3e-2 on the edited latents, what
    test_dirinv_plugin_vs_oracle / test_diffinv_plugin_vs_oracle hold at the same size."""
    import modules
    variant, p = pipe
    g = case["g"]
    inv = _inverter(p, case)
    traj = inv.invert(case["z0"], prompt=SRC, context=case["ctx"][SRC], guidance_scale_fwd=1)["latents"]
    assert len(traj) == S + 1 and all(isinstance(pr, list) and len(pr) == 2 for pr in traj)
    e_inv = rel(torch.stack([torch.cat(pr) for pr in traj]), g["inv_latents"])
    res = modules.load_editor("simple", inverter=inv).edit(case["z0"], SRC, TGT)
    assert set(res) == {"image_inv", "image", "latent_inv", "latent"} and res["image"].shape == (1, 3, 8 * L, 8 * L)
    (x,), (y,) = res["latent_inv"], res["latent"]                     # the reference's slicing of a pair: [x], [y], rows [source, target]
    e_x, e_y = rel(x, g["edit_x"]), rel(y, g["edit_y"])
    print(f"edict + simple vs oracle ({variant}): inversion rel L2 {e_inv:.3e}, edited pair rel L2 {e_x:.3e} / {e_y:.3e}")
    b_inv, b_edit = (1e-3, 1e-3) if variant == "fp32" else (5e-3, 3e-2)
    assert e_inv < b_inv and e_x < b_edit and e_y < b_edit
    assert inv._loop.rows_executed == inv._loop.expected_rows(1, 2, guidance_scale_fwd=1) + 2 * S      # (+ the first, separate inversion)


def test_round_trip_beats_plain_ddim_inversion(pipe, case):
    """invert then sample under the same context at guidance 3: EDICT returns z0, plain DDIM inversion (diffinv) does not.  The ratio of the two
    errors on the engine must reach a tenth of the ratio the CPU fp32 reference side has (edict_sd.npz); the ten is room for the engine's
    rounding against a deterministic 16-bit UNet."""
    variant, p = pipe
    g, z0, ctx = case["g"], case["z0"], case["ctx"][SRC]
    inv = _inverter(p, case)
    back = inv.sample(inv.invert(z0, context=ctx), context=ctx)["latent"]
    e_edict = er.roundtrip_error([v.double().cpu().numpy() for v in back], z0.double().cpu().numpy())
    dinv = _inverter(p, case, "diffinv", guidance_scale_fwd=3.0, guidance_scale_bwd=3.0)
    rec = dinv.sample(dinv.invert(z0, context=ctx), context=ctx)["latent"]
    e_diff = er.roundtrip_error([rec.double().cpu().numpy()], z0.double().cpu().numpy())
    want = float(g["roundtrip_diffinv"]) / float(g["roundtrip_edict"])
    print(f"round trip ({variant}): edict {e_edict:.3e}, diffinv {e_diff:.3e}, ratio {e_diff / e_edict:.3e}; "
          f"reference side: edict {float(g['roundtrip_edict']):.3e}, diffinv {float(g['roundtrip_diffinv']):.3e}, ratio {want:.3e}")
    assert e_diff / e_edict >= 0.1 * want


def test_fast_path_equals_per_step_path(pipe, case):
    """the batched device loop vs the reference-style per-step methods (predict_step_forward / predict_step_backward through the scheduler
    wrappers and sync_latent_pair), at the bound of test_per_step_plugin_path_matches_fast_path"""
    variant, p = pipe
    inv = _inverter(p, case)
    ctx_s, ctx_t = case["ctx"][SRC], case["ctx"][TGT]
    fast_inv = inv.invert(case["z0"], context=ctx_s)
    fast = inv.sample(fast_inv, context=[ctx_s, ctx_t])["latent"]
    assert "_native" in fast_inv
    inv.force_per_step = True
    slow_inv = inv.invert(case["z0"], context=ctx_s)
    slow = inv.sample(slow_inv, context=[ctx_s, ctx_t])["latent"]
    inv.force_per_step = False
    assert "_native" not in slow_inv
    for a, b in zip(slow_inv["latents"], fast_inv["latents"]):
        torch.testing.assert_close(torch.cat(a), torch.cat(b), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(torch.cat(slow), torch.cat(fast), rtol=1e-4, atol=1e-4)


def test_loop_batch_of_three_equals_single_runs(pipes, case):
    """EdictLoop at B = 3 vs three B = 1 runs, fp32, at the bounds of tests/test_batch_gpu.py (2e-3 inversion, 2e-2 edited latents)"""
    from etainv.pipeline import EdictLoop
    p = pipes("fp32")
    gen = torch.Generator().manual_seed(5)
    z0 = torch.cat([case["z0"].cpu(), 0.8 * torch.randn(2, 4, L, L, generator=gen)]).cuda()
    mk = lambda c: torch.stack([c, c + 0.05 * torch.randn(c.shape, generator=gen).cuda(), c.flip(1)]).contiguous()
    ctx_s, ctx_t = mk(case["ctx"][SRC]), mk(case["ctx"][TGT])
    loop = EdictLoop(p.engine, S=S)
    inv = loop.invert(z0, ctx_s)
    out = loop.sample(inv, [ctx_s, ctx_t])
    assert inv["latents"].shape == (S + 1, 2, 3, 4, L, L) and out.shape == (2, 6, 4, L, L)
    assert loop.rows_executed == loop.expected_rows(3, 2) == 2 * S * 3 * 2 + 2 * S * 3 * 2 * 2
    for i in range(3):
        one = EdictLoop(p.engine, S=S)
        inv1 = one.invert(z0[i:i + 1], ctx_s[i:i + 1])
        out1 = one.sample(inv1, [ctx_s[i:i + 1], ctx_t[i:i + 1]])
        e_inv, e_out = rel(inv["latents"][:, :, i:i + 1], inv1["latents"]), rel(out[:, [i, 3 + i]], out1)
        print(f"B = 3 vs B = 1, image {i}: inversion rel L2 {e_inv:.3e}, edited rel L2 {e_out:.3e}")
        assert e_inv < 2e-3 and e_out < 2e-2


def test_ptp_without_blend_runs_through_edict_controller(pipe, case, monkeypatch):
    import modules
    from modules.inversion import edict_inversion
    variant, p = pipe
    made = []

    class Recording(edict_inversion.EdictController):
        def __init__(self, controller):
            super().__init__(controller)
            made.append(self)
    monkeypatch.setattr(edict_inversion, "EdictController", Recording)
    inv = _inverter(p, case)
    cfg = dict(is_replace_controller=False, prompts=[SRC, TGT], cross_replace_steps={"default_": .4}, self_replace_steps=0.6,
               equilizer_params={"words": ("tiger",), "values": (2,)})
    res = modules.load_editor("ptp", inverter=inv).edit(case["z0"], SRC, TGT, cfg={**cfg})
    used = [c for c in made if type(c.controllers[0]).__name__ == "PromptToPromptController"]
    assert len(used) == 1 and [c.step_idx for c in used[0].controllers] == [S, S]        # each copy saw one half-step per step
    assert p.unet.attn_ctrl is None
    simple = modules.load_editor("simple", inverter=inv).edit(case["z0"], SRC, TGT)
    assert torch.isfinite(res["latent"][0]).all() and rel(res["latent"][0][1:], simple["latent"][0][1:]) > 1e-3
    with pytest.raises(NotImplementedError, match="needs a per-latent map store"):
        modules.load_editor("ptp", inverter=inv).edit(case["z0"], SRC, TGT, cfg={**cfg, "blend_words": (("cat",), ("tiger",))})
    assert p.unet.attn_ctrl is None


def test_edit_image_cli_edict(tmp_path):
    from PIL import Image
    src = tmp_path / "in.png"
    Image.fromarray((np.random.default_rng(0).random((96, 96, 3)) * 255).astype(np.uint8)).save(src)
    out = tmp_path / "out.png"
    r = subprocess.run([sys.executable, str(ROOT / "eta-inversion_amd" / "edit_image.py"), "--input", str(src), "--source_prompt", SRC,
                        "--target_prompt", TGT, "--output", str(out), "--inv_method", "edict", "--edit_method", "simple", "--steps", "3",
                        "--prec", "fp16"], capture_output=True, text=True, timeout=900,
                       env={**__import__("os").environ, "PYTHONPATH": str(ROOT / "eta-inversion_amd")})
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Saved result to" in r.stdout and "Took" in r.stdout
    assert out.exists() and (tmp_path / "out_inv.png").exists()
    assert Image.open(out).size == (512, 512)
