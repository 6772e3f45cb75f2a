"""The `pnp` editor on the engine: PNP UNet calls against tests/golden/pnp_sd.npz (tests/pnp_ref.py over the SD-width oracle UNet in float64,
16 x 16 latents, two images per call), the eta loop with pnp free-running (fp32 operands) and teacher-forced (fp16), and the plugin surface: fused path
== per-step path, BatchEditor, dirinv.

Measured on MI355X (this file's own printouts): see DESIGN.md, "Note pnp"."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import pnp_ref as pr

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
SRC, TGT = "a cat sitting next to a mirror", "a tiger sitting next to a mirror"
L, S, B = pr.SD_L, pr.SD_S, pr.SD_N_IMG
FLAGS = {"none": (False, False), "conv": (True, False), "qk": (False, True), "both": (True, True)}
FP16_UNET_TOL = 4e-3          # tests/test_unet_gpu.py: an fp16 UNet call vs the fp32 oracle at L = 16, relative L2


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm()).item()


def close32(a, b):
    """the project's tolerance for the fp32-operand mode"""
    return torch.allclose(torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu(), rtol=1e-3, atol=1e-4)


@pytest.fixture(scope="module")
def case():
    z0, ctx_src, ctx_tgt = pr.sd_case_inputs()
    lat, ctx, t = pr.sd_call_inputs()
    g = np.load(ROOT / "tests" / "golden" / "pnp_sd.npz")
    assert int(g["S"]) == S
    np.testing.assert_array_equal(torch.cat([z0.flatten()[:4], ctx_src.flatten()[-4:], ctx_tgt.flatten()[:4], lat.flatten()[-4:]]).numpy(), g["probe"])
    return dict(z0=z0.cuda(), ctx_src=ctx_src.cuda(), ctx_tgt=ctx_tgt.cuda(), lat=lat.cuda(), ctx=ctx.cuda(), t=t, g=g)


@pytest.fixture(scope="module")
def pipes():
    """variant -> pipeline, built on first use, one each for the whole module"""
    import modules
    made = {}

    def get(variant):
        if variant not in made:
            made[variant] = modules.load_diffusion_model("sd15", "cuda", variant=variant, latent_size=L, max_img=B)[0]
        return made[variant]
    yield get
    for p in made.values():
        p.engine.close()


@pytest.fixture(params=["fp32", "fp16"])
def pipe(request, pipes):
    return request.param, pipes(request.param)


def _ctrl(conv=False, qk=False, **kw):
    from etainv import _capi
    from etainv.engine import AttnControl
    return AttnControl(mode=_capi.ATTN_PNP, n_img=kw.pop("n_img", B), pnp_conv_active=conv, pnp_qk_active=qk, **kw)


def test_pnp_call_flags_off_is_the_plain_call_and_flags_on_keep_the_source_rows(pipe, case):
    """both flags 0: bit for bit the plain call on the same six rows.  A flag on: the u_s rows still are (nothing is injected INTO them), the
    target rows are not"""
    variant, p = pipe
    e = p.engine
    plain = e.unet(case["lat"], case["t"], case["ctx"]).clone()
    assert torch.equal(e.unet(case["lat"], case["t"], case["ctx"], _ctrl()), plain)
    for tag, (conv, qk) in FLAGS.items():
        if tag == "none":
            continue
        out = e.unet(case["lat"], case["t"], case["ctx"], _ctrl(conv, qk))
        assert torch.equal(out[:B], plain[:B]), tag
        d = rel(out[B:], plain[B:])
        print(f"pnp call ({variant}, {tag}): target rows differ from the plain call by rel L2 {d:.3e}")
        assert d > 1e-3, tag
    assert torch.equal(e.unet(case["lat"], case["t"], case["ctx"]), plain)                 # and the next plain call is untouched


@pytest.mark.parametrize("tag", list(FLAGS))
def test_pnp_call_vs_oracle(pipe, case, tag):
    """one UNet call per flag combination, latents distinct per image (a wrong `% n_img` would pair the wrong images)"""
    variant, p = pipe
    out = p.engine.unet(case["lat"], case["t"], case["ctx"], _ctrl(*FLAGS[tag]))
    ref = torch.from_numpy(case["g"][f"call/{tag}"])
    err, amax = rel(out, ref), float((out.cpu() - ref).abs().max())
    print(f"pnp call vs oracle ({variant}, {tag}): rel L2 {err:.3e}, max abs {amax:.3e}")
    if variant == "fp32":
        assert close32(out, ref)
    else:
        assert err < FP16_UNET_TOL


def test_bad_pnp_control_is_an_error_not_a_launch(pipes, case):
    from etainv import _capi
    e = pipes("fp16").engine
    sentinel = torch.full((3 * B, 4, L, L), 3.0, device="cuda")
    mapper = torch.zeros(B, 77, dtype=torch.int32, device="cuda")
    bad = [dict(rows=4 * B), dict(rows=3 * B, n_img=1), dict(rows=3 * B, store_maps=True), dict(rows=3 * B, mapper=mapper), dict(rows=3 * B, n_lat=2 * B)]
    for kw in bad:
        rows, n_lat = kw.pop("rows"), kw.pop("n_lat", None)
        lat = torch.cat([case["lat"], case["lat"]])[: (n_lat or rows)].contiguous()
        ctx = torch.cat([case["ctx"], case["ctx"]])[:rows].contiguous()
        out = sentinel.clone() if rows == 3 * B else torch.full((rows, 4, L, L), 3.0, device="cuda")
        with pytest.raises(_capi.EtainvError, match="plug-and-play"):
            e.unet(lat, case["t"], ctx, _ctrl(True, True, **kw), out=out)
        torch.cuda.synchronize()
        assert bool((out == 3.0).all()), kw


def _loop_inputs(case):
    g = case["g"]
    inv_lat = torch.stack([torch.from_numpy(g[f"loop/{k}/inv_latents"]) for k in range(B)], 1).cuda().contiguous()      # (S+1, B, 4, L, L)
    return g, inv_lat, torch.stack([torch.from_numpy(g[f"loop/{k}/latent"]) for k in range(B)], 1)                       # (2, B, ...) [src, tgt]


def test_eta_loop_fp32_free_running_vs_oracle(pipes, case):
    """etainv + pnp, S = 5, B = 2 (the oracle ran each image alone), fp32 operands, every step on the engine's own previous output: the
    best-of-n choice agrees at every step and the latents meet the fp32 tolerance"""
    from etainv.pipeline import EtaLoop, noise_table
    from modules.editing.pnp_editor import injection_steps
    g, inv_ref, want = _loop_inputs(case)
    loop = EtaLoop(pipes("fp32").engine, S=S, eta=pr.ETA, use_mask=False)
    inv = loop.invert(case["z0"], case["ctx_src"])
    e_inv = rel(inv["latents"], inv_ref)
    trace = []
    x = loop.sample(inv, case["ctx_src"], case["ctx_tgt"], noise_table(S, 10, L, seed=0), pnp=injection_steps(S), trace=trace)
    best = np.stack([e["best"].cpu().numpy() for e in trace], 0)                                                           # (S, B)
    d = (x[B:].cpu().double() - want[1].double()).abs()
    print(f"etainv + pnp free-running (fp32): inversion rel L2 {e_inv:.3e}, source {rel(x[:B], want[0]):.3e}, edited {rel(x[B:], want[1]):.3e}, "
          f"max abs {float(d.max()):.3e} on values up to {float(want[1].abs().max()):.1f}, share inside rtol 1e-3 / atol 1e-4 "
          f"{float((d <= 1e-4 + 1e-3 * want[1].double().abs()).double().mean()):.5f}; best-of-n {best.T.tolist()}")
    assert close32(inv["latents"], inv_ref)
    np.testing.assert_array_equal(best, np.stack([g[f"loop/{k}/best"] for k in range(B)], 1))
    assert [e["layout"] for e in trace] == ["u_s,u_t,c_t"] * 4 + ["u_t,c_t"] and loop.rows_executed == B * S + B * (4 * 3 + 2)
    assert close32(x[:B], want[0]) and close32(x[B:], want[1])


def test_eta_loop_fp16_teacher_forced_vs_oracle(pipes, case):
    """the same loop with fp16 operands, every step started from the oracle's latents (a discontinuous argmin neither hides nor fakes a
    failure): the rows each step ran, against the oracle's, at the bound of an fp16 UNet call; the last step is past both windows and its
    source row is replayed, so it runs [u_t, c_t]"""
    from etainv.pipeline import EtaLoop, noise_table
    from modules.editing.pnp_editor import injection_steps
    g, inv_ref, _ = _loop_inputs(case)
    bwd = torch.stack([torch.from_numpy(g[f"loop/{k}/bwd_latents"]) for k in range(B)], 2).cuda()                         # (S, 2, B, 4, L, L)
    teacher = torch.cat([torch.stack([inv_ref[S], inv_ref[S]])[None], bwd[:-1]]).reshape(S, 2 * B, 4, L, L).contiguous()
    eps_ref = torch.stack([torch.from_numpy(g[f"loop/{k}/eps_rows"]) for k in range(B)], 2)                              # (S, 3, B, 4, L, L)
    flags = g["loop/0/flags"].tolist()
    assert flags == [[int(c), int(q)] for c, q in pr.step_flags(S)] == g["loop/1/flags"].tolist()
    loop = EtaLoop(pipes("fp16").engine, S=S, eta=pr.ETA, use_mask=False)
    trace = []
    loop.sample({"latents": inv_ref, "maps_mean": None}, case["ctx_src"], case["ctx_tgt"], noise_table(S, 10, L, seed=0), pnp=injection_steps(S),
                trace=trace, teacher=teacher)
    for i, e in enumerate(trace):
        want = eps_ref[i] if e["layout"] == "u_s,u_t,c_t" else eps_ref[i, 1:]
        assert e["layout"] == ("u_s,u_t,c_t" if i < S - 1 else "u_t,c_t") and e["eps_rows"].shape[0] == want.shape[0] * B
        err = rel(e["eps_rows"], want.reshape(-1, 4, L, L))
        print(f"etainv + pnp teacher-forced (fp16) step {i} t={e['t']} flags {flags[i]} rows {e['layout']}: rel L2 {err:.3e}")
        assert err < FP16_UNET_TOL, i


def _inverter(p, case, name, **kw):
    """the inverter fed with the case's latent and contexts directly (the VAE and the text encoder are tested elsewhere)"""
    import modules
    inv = modules.load_inverter(name, model=p, scheduler="ddim", num_inference_steps=S, **kw)
    ctx = {SRC: case["ctx_src"][0], TGT: case["ctx_tgt"][0]}                    # ([negative prompt, target] is what the editor asks for)
    inv.encode = lambda image: image.to("cuda").float()
    inv.create_context = lambda prompt, negative_prompt="": ctx[prompt]
    return inv


def test_dirinv_plugin_vs_oracle(pipes, case):
    """load_editor("pnp", inverter=dirinv).edit on fp32 operands vs the oracle's eta = 0 loop under the hooks"""
    import modules
    inv = _inverter(pipes("fp32"), case, "dirinv")
    res = modules.load_editor("pnp", inverter=inv).edit(case["z0"][:1], SRC, TGT)
    assert set(res) == {"image_inv", "image", "latent_inv", "latent"} and res["image"].shape == (1, 3, 8 * L, 8 * L)
    want = torch.from_numpy(case["g"]["dirinv/latent"])
    print(f"dirinv + pnp vs oracle (fp32): source rel L2 {rel(res['latent_inv'], want[:1]):.3e}, edited rel L2 {rel(res['latent'], want[1:]):.3e}")
    assert close32(res["latent_inv"], want[:1]) and close32(res["latent"], want[1:])
    assert pipes("fp32").unet.attn_ctrl is None


@pytest.mark.parametrize("name", ["etainv", "diffinv"])
def test_plugin_fused_path_equals_per_step_path(pipes, case, name):
    """edit() through the batched device loop vs the reference-style per-step path (PnpController.begin_step -> the UNet wrapper's 4 -> 3 -> 4
    rows -> step -> end_step), compared the way tests/test_modules_api_gpu.py compares the two paths of the other editors; diffinv has only the
    per-step path and must run it under the same hooks"""
    import modules
    p = pipes("fp16")
    kw = dict(eta=(0.3, 0.6)) if name == "etainv" else {}
    inv = _inverter(p, case, name, **kw)
    editor = modules.load_editor("pnp", inverter=inv)
    cfg = dict(inv_cfg=dict(edit_word_idx=(1, 1))) if name == "etainv" else {}
    fast = editor.edit(case["z0"][:1], SRC, TGT, **cfg)
    assert set(fast) == {"image_inv", "image", "latent_inv", "latent"} and torch.isfinite(fast["latent"]).all()
    assert p.unet.attn_ctrl is None
    if name == "diffinv":
        plain = modules.load_editor("simple", inverter=inv).edit(case["z0"][:1], SRC, TGT)
        assert rel(fast["latent"], plain["latent"]) > 1e-3                       # (same contexts: the injections alone make the difference)
        return
    inv.force_per_step = True
    slow = editor.edit(case["z0"][:1], SRC, TGT, **cfg)
    inv.force_per_step = False
    torch.testing.assert_close(slow["latent_inv"], fast["latent_inv"], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(slow["latent"], fast["latent"], rtol=1e-4, atol=1e-4)
    assert p.unet.attn_ctrl is None


def test_batch_editor_equals_single_runs(pipes):
    """BatchEditor("pnp") at B = 2 vs load_editor("pnp").edit one image at a time, under the rule of tests/test_batch_gpu.py"""
    from etainv.batch import BatchEditor
    from modules import load_editor, load_inverter
    p = pipes("fp16")
    g = torch.Generator().manual_seed(12)
    samples = [dict(image=torch.rand(1, 3, 8 * L, 8 * L, generator=g) * 2 - 1, source_prompt=s, target_prompt=t, edit_word_idx=[1, 1], ptp=None)
               for s, t in ((SRC, TGT), ("a round cake with orange frosting", "a square cake with orange frosting"))]
    batch = BatchEditor(p, num_inference_steps=4, edit_method="pnp").edit(samples)
    editor = load_editor("pnp", inverter=load_inverter("etainv", model=p, scheduler="ddim", num_inference_steps=4, eta=[[0.6, 0], [1, 0.7]]))
    for s, got in zip(samples, batch):
        want = editor.edit(s["image"].cuda(), s["source_prompt"], s["target_prompt"], inv_cfg=dict(edit_word_idx=s["edit_word_idx"]))
        print(f"BatchEditor pnp vs single: source {rel(got['latent_inv'], want['latent_inv']):.3e}, edited {rel(got['latent'], want['latent']):.3e}")
        assert rel(got["latent_inv"], want["latent_inv"]) < 2e-3
        assert rel(got["latent"], want["latent"]) < 2e-2
        assert got["image"].shape == (1, 3, 8 * L, 8 * L) and rel(got["image"], want["image"]) < 2e-2
