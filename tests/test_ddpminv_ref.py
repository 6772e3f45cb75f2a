"""tests/ddpminv_ref.py (the float64 reference of the native ddpminv / cyclediff inverters) against fixtures recorded from the reference
implementation's own DDPMInverseScheduler / DDPMInversion (tests/golden/make_ddpminv_golden.py --reference).  No GPU."""
from pathlib import Path

import numpy as np
import pytest

from tests import ddpminv_ref as dr

ROOT = Path(__file__).resolve().parents[1]
MODES = {"ddpminv": False, "cyclediff": True}


def golden(name):
    return np.load(ROOT / "tests" / "golden" / f"{name}.npz")


@pytest.mark.parametrize("tag", list(MODES))
@pytest.mark.parametrize("S", [1, 5])
def test_sample_latents_and_step_match_the_reference(S, tag):
    """L = 8: the arrays.  float64: the same arithmetic on the same table, so a few ulps; float32: each operation rounds where torch's does, but the
    coefficients come from float64 (the reference forms them in fp32), so a few fp32 ulps of the largest term"""
    g, L = golden("ddpm_inverse"), 8
    x0, noise, eps = dr.kernel_case(S, L)
    np.testing.assert_array_equal(np.concatenate([x0.ravel()[:4], noise.ravel()[:4], eps.ravel()[:4]]), g[f"S{S}_L{L}/probe"])
    key = f"S{S}_L{L}/{tag}"
    xts = dr.sample_latents(x0, noise, S, MODES[tag])
    assert xts.shape == (S + 1, 1, 4, L, L) and np.array_equal(xts[S], x0)
    np.testing.assert_allclose(xts[:, 0], g[f"{key}/xts_f64"], rtol=1e-13, atol=1e-14)
    xts32 = dr.sample_latents(x0, noise, S, MODES[tag], dtype=np.float32)
    assert xts32.dtype == np.float32
    np.testing.assert_allclose(xts32[:, 0], g[f"{key}/xts_f32"], rtol=0, atol=4 * 2.0 ** -24 * np.abs(g[f"{key}/xts_f64"]).max())
    xin = g[f"{key}/xts_f32"][:, None]                               # the step runs on the float32 run's noised latents in both types
    for i, t in enumerate(dr.timesteps(S)):
        idx = S - 1 - i
        coef = dr.step_coefficients(S, t)
        z, prev, mu = dr.inverse_step(xin[idx], xin[idx + 1], eps[i], coef)
        if t == 0:
            # the deliberate deviation: the reference divides by zero here (its values are not finite), the restatement returns z = 0 and mu
            assert coef[4] == 0 and not np.isfinite(g[f"{key}/z_f64"][i]).all()
            assert not z.any() and np.array_equal(prev, mu) and np.isfinite(mu).all()
            continue
        np.testing.assert_allclose(z, g[f"{key}/z_f64"][i], rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(prev, g[f"{key}/prev_f64"][i], rtol=1e-12, atol=1e-13)
        z32, prev32, _ = dr.inverse_step(xin[idx], xin[idx + 1], eps[i], coef, dtype=np.float32)
        scale = np.abs(xin[idx]).max() + np.abs(eps[i]).max()
        np.testing.assert_allclose(prev32, g[f"{key}/prev_f32"][i], rtol=0, atol=8 * 2.0 ** -24 * scale)
        np.testing.assert_allclose(z32, g[f"{key}/z_f32"][i], rtol=0, atol=8 * 2.0 ** -24 * scale / coef[4])


def test_yardstick_is_float32_rounding():
    """the float32-against-float64 distances the GPU kernel tests scale their bounds from: all cases present, all at the size of fp32 rounding"""
    g = golden("ddpm_inverse")
    for S, L in dr.KERNEL_CASES:
        for tag in MODES:
            names = ["err_xts"] + (["err_z", "err_prev"] if S > 1 else [])
            for n in names:
                v = float(g[f"S{S}_L{L}/{tag}/{n}"])
                assert 1e-8 < v < 3e-7, (S, L, tag, n, v)


@pytest.mark.parametrize("tag", list(MODES))
def test_e2e_matches_the_reference(tag):
    """DdpmInvRef over the toy-width oracle UNet (float64) against the reference's fp32 run of invert + sample([source, target]) on the noise it
    drew.  The noise maps amplify the UNet's rounding by |c_eps| / sigma, so they are held to the exact relation instead: recomputed in float64
    from the fixture's own noise predictions they must agree with the fixture's at fp32 rounding."""
    from oracle.unet import build_unet
    from tests.edict_ref import torch_unet
    g, d = golden("e2e_ddpminv"), golden("e2e_diffinv")
    ctx_s, ctx_t = d["ctx_src"], d["ctx_tgt"]
    np.testing.assert_array_equal(np.concatenate([ctx_s.ravel()[:4], ctx_t.ravel()[-4:]]), g["ctx_probe"])
    S = int(g["S"])
    assert S == 5 and dr.bwd_skip(S) == 1
    toy = torch_unet(build_unet(0, block_out_channels=(32, 64, 128, 128)).double())
    ref = dr.DdpmInvRef(toy, S, markovian=MODES[tag])
    inv = ref.invert(g["z0"], ctx_s, g[f"{tag}/noise"])
    np.testing.assert_allclose(inv["noise_preds"][:, 0], g[f"{tag}/noise_preds"], rtol=1e-4, atol=2e-5)
    assert not np.isfinite(g[f"{tag}/latents"][0]).all()                                       # the reference's t = 0 latent: divided by zero
    np.testing.assert_allclose(inv["latents"][1:, 0], g[f"{tag}/latents"][1:], rtol=1e-4, atol=2e-5)
    assert not inv["zs"][0].any() and not g[f"{tag}/zs"][0].any()
    for i, t in enumerate(dr.timesteps(S)):
        if i == 0:
            continue
        coef, idx = dr.step_coefficients(S, t), S - 1 - i
        z = dr.inverse_step(inv["xts"][idx, 0], inv["xts"][idx + 1, 0], g[f"{tag}/noise_preds"][i], coef)[0]
        scale = np.abs(inv["xts"][idx]).max() + np.abs(g[f"{tag}/noise_preds"][i]).max()
        np.testing.assert_allclose(z, g[f"{tag}/zs"][i], rtol=0, atol=16 * 2.0 ** -24 * scale / coef[4])
    edit = ref.sample(inv, [ctx_s, ctx_t])
    np.testing.assert_allclose(edit, g[f"{tag}/edit"], rtol=1e-3, atol=2e-4)
    assert np.abs(edit[1] - edit[0]).max() > 1e-2                                              # the two rows differ: prompts and scales


def test_skip_of_zero_skips_nothing():
    calls = []

    def unet(x, t, ctx):
        calls.append(int(t))
        return np.zeros_like(x)
    S = 2                                                                                      # int(0.36 * 2) == 0
    ref = dr.DdpmInvRef(unet, S)
    z0, noise = np.ones((1, 4, 8, 8)), np.ones((S, 1, 4, 8, 8))
    ctx = np.zeros((2, 77, 768))
    inv = ref.invert(z0, ctx, noise)
    calls.clear()
    out = ref.sample(inv, [ctx, ctx])
    assert calls == [500, 0] and out.shape == (2, 4, 8, 8) and np.isfinite(out).all()
