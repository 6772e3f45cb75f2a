"""Plug-and-play, CPU side: tests/pnp_ref.py (the hooks restated on the oracle's UNet, what the GPU tests compare the engine with) against
fixtures recorded from the reference implementation's own PlugAndPlayEditor / register_pnp (tests/golden/make_pnp_golden.py --reference); the
step windows of the plugin and the row economy of EtaLoop.sample(pnp=...) against the same fixtures; the registry."""
import contextlib
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import loop as oloop
from oracle import schedule as sch
from tests import pnp_ref as pr
from tests.golden.make_pnp_golden import E2E_S, ETA, SCHEDULE_S


@pytest.fixture(scope="module")
def toy():
    from oracle.unet import build_unet
    return build_unet(0, block_out_channels=(32, 64, 128, 128))


def _contexts(g):
    """the generator's stand-in tokenizer and text encoder (no reference code involved): [uncond, source], [negative prompt, target]"""
    from tests.golden.make_golden import FakeTokenizer, text_embed
    src, tgt = json.load(open(Path(__file__).parent / "golden" / "prompt_pairs.json"))[0]
    emb = lambda p: text_embed(FakeTokenizer()([p]).input_ids)[0]
    ctx_s, ctx_t = torch.stack([emb(""), emb(src)]), torch.stack([emb(pr.NEGATIVE_PROMPT), emb(tgt)])
    probe = torch.cat([ctx_s.flatten()[:4], ctx_s.flatten()[-4:], ctx_t.flatten()[:4], ctx_t.flatten()[-4:]])
    np.testing.assert_array_equal(probe.numpy(), g["ctx_probe"])
    return src, ctx_s, ctx_t


@pytest.mark.parametrize("tag", ["etainv", "dirinv"])
def test_e2e_vs_reference(golden, toy, tag):
    """pnp_sample_ref over the toy oracle UNet vs the reference's PlugAndPlayEditor on etainv (paper eta schedule, S = 5: steps with eta > 0, steps
    with eta == 0 under a live injection, and a last step with neither) and on dirinv.  The same network in fp32 on the CPU, differing by operation
    order: the bound tests/test_edict_ref.py and tests/test_oracle_golden.py hold their e2e comparisons to (rtol 1e-3, atol 2e-4).
    Measured max |diff|: etainv source 2.4e-7, target 1.27e-4; dirinv source 2.4e-7, target 1.28e-4 (latents of magnitude ~3)."""
    g = golden("e2e_pnp")
    S = int(g["S"])
    assert S == E2E_S
    src, ctx_s, ctx_t = _contexts(g)
    z0 = torch.from_numpy(g["z0"])
    with torch.no_grad():
        if tag == "etainv":
            o, n_cand = oloop.EtaInversionOracle(toy, S=S, eta=ETA), 10
        else:
            o, n_cand = oloop.EtaInversionOracle(toy, S=S, eta=(0.0, 0.0), noise_sample_count=1, use_mask=False), 1
        inv = o.invert(z0, ctx_s, src)
        if tag == "etainv":
            np.testing.assert_allclose(inv["latents"][-1].numpy(), g["zT_inv"], rtol=1e-4, atol=2e-5)
        trace = []
        z = pr.pnp_sample_ref(o, inv, ctx_s, ctx_t, oloop.noise_table(S, n_cand, 64, seed=0), edit_word_idx=(1, 1), trace=trace)
    calls = g[f"{tag}/calls"]
    assert [e["t"] for e in trace] == calls[:, 0].tolist() and calls[:, 3].tolist() == list(range(1, S + 1))   # one hooked call per step
    assert [[int(e["conv"]), int(e["qk"])] for e in trace] == calls[:, 1:3].tolist()                     # what the hooked modules did, step by step
    print(f"{tag}: max |diff| source {np.abs(z[:1].numpy() - g[f'{tag}/latent_inv']).max():.2e} target {np.abs(z[1:].numpy() - g[f'{tag}/latent']).max():.2e}")
    np.testing.assert_allclose(z[:1].numpy(), g[f"{tag}/latent_inv"], rtol=1e-3, atol=2e-4)
    np.testing.assert_allclose(z[1:].numpy(), g[f"{tag}/latent"], rtol=1e-3, atol=2e-4)


@pytest.mark.parametrize("S", SCHEDULE_S)
def test_step_windows_vs_reference(golden, S):
    """which backward steps fire the conv hook and the Q/K hooks: recorded from the reference's hooked modules after its own register_pnp /
    register_time, exact for every step; pnp_ref and the plugin's arithmetic both have to give that table"""
    from modules.editing.pnp_editor import injection_steps
    rows = golden("pnp_schedule")[f"S{S}"]
    assert rows[:, 0].tolist() == [int(t) for t in sch.timesteps_backward(S)]
    assert [[int(c), int(q)] for c, q in pr.step_flags(S)] == rows[:, 1:].tolist()
    conv_steps, qk_steps = injection_steps(S)
    assert (conv_steps, qk_steps) == pr.windows(S) == (int(rows[:, 1].sum()), int(rows[:, 2].sum()))
    assert rows[:conv_steps, 1].all() and rows[:qk_steps, 2].all()                                       # (leading steps, no gaps)


class _FakeLib:
    def __getattr__(self, name):
        return lambda *a, **k: 0


class _FakeEngine:
    """recorder in place of the engine, as tests/test_host_logic.py drives EtaLoop; every UNet call fills output row r with r + 1"""
    L, lib, map_div = 8, _FakeLib(), 4

    def __init__(self):
        self.calls = []

    def unet(self, latent, t, ctx, ctrl=None, out=None):
        c = ctrl.c if ctrl is not None else None
        self.calls.append(dict(rows=ctx.shape[0], n_lat=latent.shape[0], t=int(t), mode=c.mode if c else 0, n_img=c.n_img if c else 0,
                               conv=bool(c.pnp_conv_active) if c else False, qk=bool(c.pnp_qk_active) if c else False,
                               clean=c is None or (c.store_maps == 0 and c.first_row == 0 and c.src_exit_block == 0 and not c.mapper and not c.cross_alpha),
                               latent=latent.clone()))
        out.copy_(torch.arange(1, ctx.shape[0] + 1, dtype=out.dtype).reshape(-1, 1, 1, 1).expand_as(out))
        return out

    def maps_reset(self): pass
    def maps_configure(self, div): self.map_div = div
    def word_maps_ex(self, *a, **k): pass

    @contextlib.contextmanager
    def cached_context(self):
        yield


@pytest.mark.parametrize("S", SCHEDULE_S)
def test_loop_rows_and_flags_host_logic(golden, monkeypatch, S):
    """EtaLoop.sample(pnp=<the plugin's windows>) against the reference's table: every step with eta > 0 or a live injection runs 3 B rows
    [u_s, u_t, c_t] over 3 B latents [src, tgt, tgt] under an ATTN_PNP control with exactly the recorded flags; a step with eta == 0 past both
    windows runs the plain 2 B rows [u_t, c_t]; skip_dead_source_rows=False runs 3 B everywhere; the noise rows reach the step kernel as
    [u_s, u_t, u_s, c_t]."""
    from etainv import _capi
    from etainv.flops import pnp_step_rows
    from etainv.pipeline import EtaLoop
    from modules.editing.pnp_editor import injection_steps
    monkeypatch.setattr(_capi, "ptr", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(_capi, "stream_ptr", lambda: None)
    monkeypatch.setattr(_capi, "check", lambda rc: None)
    rows = golden("pnp_schedule")[f"S{S}"]
    B, L = 2, 8
    inv = {"latents": torch.arange(S + 1, dtype=torch.float32).reshape(-1, 1, 1, 1, 1).expand(S + 1, B, 4, L, L).contiguous(), "maps_mean": None, "maps_steps": None}
    ctx_s, ctx_t = torch.zeros(B, 2, 77, 768), torch.ones(B, 2, 77, 768)
    noise = torch.zeros(S, 10, 4, L, L)

    def run(**kw):
        eng, trace = _FakeEngine(), []
        loop = EtaLoop(eng, S=S, eta=ETA, use_mask=False, **kw)
        loop.sample(inv, ctx_s, ctx_t, noise, pnp=injection_steps(S), trace=trace)
        return eng.calls, loop, trace
    calls, loop, trace = run()
    eta_zero = [float(loop.etas[int(t)]) == 0.0 for t in rows[:, 0]]
    assert any(eta_zero) and not all(eta_zero)
    want = [3 * B if (not z or c or q) else 2 * B for (t, c, q), z in zip(rows.tolist(), eta_zero)]
    assert want == [r * B for r in pr.step_rows(S, eta_zero)] == [pnp_step_rows(i, B, *injection_steps(S), z) for i, z in enumerate(eta_zero)]
    assert 2 * B in want and [c["rows"] for c in calls] == want and [c["t"] for c in calls] == rows[:, 0].tolist()
    assert loop.rows_executed == sum(want)
    for c, (t, conv, qk), e in zip(calls, rows.tolist(), trace):
        if c["rows"] == 3 * B:
            assert (c["mode"], c["n_img"], c["n_lat"], c["clean"]) == (_capi.ATTN_PNP, B, 3 * B, True)
            assert (c["conv"], c["qk"]) == (bool(conv), bool(qk))
            assert torch.equal(c["latent"][B:2 * B].view(torch.int32), c["latent"][2 * B:].view(torch.int32))   # latents [src, tgt, tgt] (bits: the fake step kernel leaves them unwritten)
            assert e["layout"] == "u_s,u_t,c_t"
        else:
            assert (c["mode"], c["n_lat"], conv, qk, e["layout"]) == (0, B, 0, 0, "u_t,c_t")
        if e["eps_all"] is not None:                                                                     # rows [0, 1, 0, 2] of the three-row call
            assert e["eps_all"].reshape(4, B, -1)[:, :, 0].tolist() == [[1, 2], [3, 4], [1, 2], [5, 6]]
    calls, loop, _ = run(skip_dead_source_rows=False)
    assert [c["rows"] for c in calls] == [3 * B] * S and loop.rows_executed == 3 * B * S
    assert [(c["conv"], c["qk"]) for c in calls] == [(bool(c_), bool(q_)) for _, c_, q_ in rows.tolist()]
    with pytest.raises(ValueError, match="exclusive"):
        EtaLoop(_FakeEngine(), S=S, eta=ETA, use_mask=False).sample(inv, ctx_s, ctx_t, noise, pnp=injection_steps(S), masactrl=(4, 10))


def test_guided_source_noise_is_uncond_source_noise(toy):
    """the wrapper returns the uncond source noise in the cond source row's place, so classifier-free guidance on the source rows, u + g (c - u),
    is u_s bit for bit -- at any guidance scale"""
    g = torch.Generator().manual_seed(5)
    lat, ctx = torch.randn(2, 4, 8, 8, generator=g), torch.randn(4, 77, 768, generator=g)
    hooked = pr.PnpUNet(toy, 1)
    hooked.conv_on = hooked.qk_on = True
    with torch.no_grad(), hooked.hooked():
        eps = hooked(torch.cat([lat, lat]), torch.tensor(601), encoder_hidden_states=ctx)["sample"]
        three = hooked.rows3(torch.cat([lat, lat[1:]]), torch.tensor(601), ctx[[0, 1, 3]])
    assert hooked.fired == {"conv": 2, "qk": 16}
    assert "forward" not in vars(hooked.conv_site) and all("forward" not in vars(m) for m in hooked.attn_sites)   # hooks gone
    assert torch.equal(eps[2], eps[0]) and torch.equal(eps[[0, 1, 3]], three)
    for scale in (7.5, 3.0, 1.0):
        assert torch.equal(eps[0] + scale * (eps[2] - eps[0]), eps[0])
    with torch.no_grad():
        plain = toy(torch.cat([lat, lat[1:]]), torch.tensor(601), encoder_hidden_states=ctx[[0, 1, 3]])["sample"]
    assert torch.equal(plain[0], three[0]) and not torch.allclose(plain[1:], three[1:], atol=1e-4)        # the source row is untouched, the targets are not


def test_registry_and_inverter_check():
    """`pnp` is a built editor; it checks its inverter when it is constructed: etainv, dirinv and diffinv pass, edict and anything else
    (None included) is refused with a message that names what it is built for"""
    import types
    import modules
    from modules.editing.pnp_editor import PlugAndPlayEditor
    from modules.inversion.diffusion_inversion import DiffusionInversion
    from modules.inversion.direct_inversion import DirectInversion
    from modules.inversion.edict_inversion import EdictInversion
    from modules.inversion.eta_inversion import EtaInversion
    assert "pnp" in modules.get_edit_methods() and modules._editors["pnp"] is PlugAndPlayEditor
    for cls in (EtaInversion, DirectInversion, DiffusionInversion):
        inv = object.__new__(cls)
        inv.model = types.SimpleNamespace()
        ed = modules.load_editor("pnp", inverter=inv)
        assert isinstance(ed, PlugAndPlayEditor) and ed.negative_prompt == pr.NEGATIVE_PROMPT and ed.no_null_source_prompt
    for bad in (object.__new__(EdictInversion), None):
        with pytest.raises(NotImplementedError, match="etainv, dirinv and diffinv"):
            modules.load_editor("pnp", inverter=bad)
    with pytest.raises(NotImplementedError, match="simple, ptp, masactrl, pnp"):
        modules.load_editor("pix2pix_zero", inverter=None)
