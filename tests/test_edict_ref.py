"""tests/edict_ref.py (the numpy restatement of EDICT that the GPU tests compare the engine with) against fixtures recorded from the reference
implementation's own EdictScheduler / EdictSchedulerInverse / EdictInversion (tests/golden/make_edict_golden.py --reference).  CPU only."""
import numpy as np
import pytest
import torch

from tests import edict_ref as er
from tests.golden.make_edict_golden import PTP_CFG, STEP_CASES, step_case_inputs


@pytest.mark.parametrize("S,strength,leap", STEP_CASES)
def test_order_tables_and_timesteps(golden, S, strength, leap):
    g = golden("edict_steps")
    key = f"S{S}_s{strength}_l{int(leap)}"
    t_fwd, t_bwd = er.timesteps(S, strength)
    np.testing.assert_array_equal(t_fwd, g[f"{key}/t_fwd"])
    np.testing.assert_array_equal(t_bwd, g[f"{key}/t_bwd"])
    np.testing.assert_array_equal(np.array([er.order(i, S, True, leap) for i in range(len(t_fwd))]), g[f"{key}/order_fwd"])
    np.testing.assert_array_equal(np.array([er.order(i, S, False, leap) for i in range(len(t_bwd))]), g[f"{key}/order_bwd"])


@pytest.mark.parametrize("S", [3, 4, 50])
def test_coefficients(golden, S):
    """a, b, abar_t, abar_prev of every timestep, both directions; S = 3 has the fractional previous timestep (interpolated table entries)"""
    g = golden("edict_steps")
    ac = er.alphas_cumprod32()
    for tag, inverse in (("fwd", True), ("bwd", False)):
        got = np.array([[float(v) for v in er.coefficients(ac, int(t), S, inverse)] for t in g[f"S{S}/t_{tag}"]])
        np.testing.assert_allclose(got, g[f"S{S}/coef_{tag}"], rtol=1e-6, atol=0)
    if S == 3:       # the interpolation really is the reversed one: 666 - 333.33 = 332.67 weighs table entry 332 with 0.67
        a_p = float(er.alpha_at(ac, np.float32(666 - 1000 / 3)))
        assert abs(a_p - (0.6667 * ac[332] + 0.3333 * ac[333])) < abs(a_p - (0.3333 * ac[332] + 0.6667 * ac[333]))


@pytest.mark.parametrize("S,strength,leap", STEP_CASES)
def test_one_step_each_way(golden, S, strength, leap):
    """a full inversion step and a full denoising step (un-mix / two coupled updates in order / mix) at guidance 3 over a constant-eps UNet"""
    g = golden("edict_steps")
    key = f"S{S}_s{strength}_l{int(leap)}"
    x, y, eps = (v.numpy() for v in step_case_inputs(S))
    if f"S{S}/probe" in g.files:
        np.testing.assert_array_equal(np.concatenate([x.ravel()[:4], y.ravel()[:4], eps.ravel()[:4]]), g[f"S{S}/probe"])
    ref = er.EdictRef(lambda lat, t, ctx: eps, S, leapfrog_steps=leap, init_image_strength=strength)
    ctx = np.zeros((2, 77, 8))
    fwd = ref.step_forward([x, y], int(g[f"{key}/step_fwd_index"]), ctx)
    bwd = ref.step_backward([x, y], 0, ctx)
    np.testing.assert_allclose(np.stack(fwd), g[f"{key}/step_fwd"], rtol=1e-5, atol=0)
    np.testing.assert_allclose(np.stack(bwd), g[f"{key}/step_bwd"], rtol=1e-5, atol=0)


@pytest.fixture(scope="module")
def toy():
    from oracle.unet import build_unet
    return build_unet(0, block_out_channels=(32, 64, 128, 128))


def _contexts(golden):
    """the prompt embeddings of the e2e fixtures: stored once, in e2e_diffinv.npz (same prompts, same stand-in text encoder)"""
    d, g = golden("e2e_diffinv"), golden("e2e_edict")
    np.testing.assert_array_equal(np.concatenate([d["ctx_src"].ravel()[:4], d["ctx_tgt"].ravel()[-4:]]), g["ctx_probe"])
    return d["ctx_src"], d["ctx_tgt"]


def test_e2e_simple_vs_reference(golden, toy):
    """EdictRef over the toy oracle UNet vs the reference's EdictInversion + SimpleEditor (inversion at guidance 1, the editor's argument; backward
    pass over [source, target] at guidance 3), at the bounds tests/test_oracle_golden.py holds e2e_diffinv to"""
    g, (ctx_s, ctx_t) = golden("e2e_edict"), _contexts(golden)
    ref = er.EdictRef(er.torch_unet(toy), int(g["S"]))
    traj = ref.invert(g["z0"], ctx_s, g=1)
    np.testing.assert_allclose(np.stack([np.concatenate(p) for p in traj[1:]]), g["simple/inv_latents"], rtol=1e-4, atol=2e-5)
    x, y = ref.sample(traj[-1], [ctx_s, ctx_t])
    np.testing.assert_allclose(x, g["simple/latent_inv"], rtol=1e-3, atol=2e-4)
    np.testing.assert_allclose(y, g["simple/latent"], rtol=1e-3, atol=2e-4)


def test_e2e_ptp_vs_reference(golden, toy):
    """the same with prompt-to-prompt (no LocalBlend): one controller per pair member, each advanced by its own half-steps (EdictController)"""
    from oracle import ptp as optp
    from oracle.loop import ptp_hook
    g, (ctx_s, ctx_t) = golden("e2e_edict"), _contexts(golden)
    S = int(g["S"])
    pairs = __import__("json").load(open(__import__("pathlib").Path(__file__).parent / "golden" / "prompt_pairs.json"))
    src, tgt = pairs[0]
    ctl = [optp.make_edit_controller(src, tgt, S, optp.WordTokenizer(), **PTP_CFG) for _ in range(2)]
    ref = er.EdictRef(er.torch_unet(toy), S)
    traj = ref.invert(g["z0"], ctx_s)                                               # the controller-based editors invert at the inverter's guidance 3

    def end_step(k, latent):
        out = ctl[k].step_callback(torch.from_numpy(latent)).numpy()
        toy.set_ctrl(None)
        return out
    try:
        x, y = ref.sample(traj[-1], [ctx_s, ctx_t], begin_step=lambda k: toy.set_ctrl(ptp_hook(ctl[k])), end_step=end_step)
    finally:
        toy.set_ctrl(None)
    np.testing.assert_allclose(x, g["ptp/latent_inv"], rtol=1e-3, atol=2e-4)
    np.testing.assert_allclose(y, g["ptp/latent"], rtol=1e-3, atol=2e-4)
    assert np.abs(y - g["simple/latent"]).max() > 1e-3                              # and the attention edit really changes the result
