"""Host-side pieces of the ddpminv / cyclediff inverters: the plugin surface against the reference's signatures, the C-ABI table, the refusal
of a model without an engine, the registry, the chunk plan of the time-parallel inversion and the UNet row count.  No GPU."""
import ctypes
import inspect
import types
from functools import partial
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("etainv_ddpm_sample_latents", "etainv_ddpm_invert_steps", "etainv_ddpm_backward_step")


def test_signatures_and_defaults_mirror_the_reference():
    """reference modules/inversion/ddpm_inversion.py:14-20 and modules/inverse_schedulers/ddpm_inverse_scheduler.py:17,35,86,156"""
    from modules.inversion.ddpm_inversion import DDPMInversion
    from modules.inverse_schedulers import DDPMInverseScheduler
    from modules.inversion.diffusion_inversion import DiffusionInversion
    assert issubclass(DDPMInversion, DiffusionInversion)
    assert (DDPMInversion.dft_skip_steps, DDPMInversion.dft_forward_seed) == (0.36, 0)
    p = inspect.signature(DDPMInversion.__init__).parameters
    assert list(p) == ["self", "model", "scheduler", "num_inference_steps", "guidance_scale_bwd", "guidance_scale_fwd", "verbose", "forward_seed",
                       "skip_steps", "markovian_forward"]
    assert [p[k].default for k in list(p)[2:]] == [None, None, None, None, False, 0, None, False]
    for name in ("create_schedulers", "predict_step_forward", "diffusion_forward", "skip_inv_result", "get_bwd_skip", "sample",
                 "predict_step_backward", "diffusion_backward"):
        assert name in vars(DDPMInversion), name
    assert list(inspect.signature(DDPMInversion.predict_step_forward).parameters) == ["self", "latent", "t", "context", "guidance_scale_fwd", "xts"]
    assert list(inspect.signature(DDPMInversion.predict_step_backward).parameters) == ["self", "latent", "t", "context", "eta", "variance_noise",
                                                                                       "guidance_scale_bwd"]
    s = inspect.signature(DDPMInverseScheduler.__init__).parameters
    assert list(s) == ["self", "scheduler", "inv_steps", "eta", "markovian_forward"]
    assert [s[k].default for k in list(s)[2:]] == ["sameshift", 1, False]
    f = inspect.signature(DDPMInverseScheduler.from_scheduler).parameters
    assert list(f) == ["scheduler", "inv_steps", "markovian_forward", "kwargs"] and f["inv_steps"].default == "sameshift"
    sl = inspect.signature(DDPMInverseScheduler.sample_latents).parameters
    assert list(sl) == ["self", "latent", "generator", "noise"] and sl["generator"].default is None and sl["noise"].default is None
    assert list(inspect.signature(DDPMInverseScheduler.step).parameters) == ["self", "noise_pred", "t", "latent", "xts"]
    assert DDPMInverseScheduler.Output._fields == ("prev_sample", "variance_noise")
    for name in ("set_timesteps", "timesteps", "get_variance", "get_sampled_latent_by_t", "get_eta_by_t"):
        assert name in vars(DDPMInverseScheduler), name


def test_new_symbols_are_declared_listed_and_exported():
    from etainv import _capi
    header = (ROOT / "include" / "etainv.h").read_text()
    lib = ctypes.CDLL(str(_capi.lib_path()))
    for name in NEW_SYMBOLS:
        assert name in _capi.SIGNATURES, name
        assert f"int {name}(" in header, name
        assert hasattr(lib, name), name
    assert "ddpm_inverse_scheduler.py:86-129" in header and "ddpm_inverse_scheduler.py" in header and "ddpm_inversion.py:135-166" in header
    assert lib.etainv_abi_version() == 1
    # argument counts of the table = those of the header's declarations
    for name in NEW_SYMBOLS:
        decl = header.split(f"int {name}(", 1)[1].split(");", 1)[0]
        assert len(decl.split(",")) == len(_capi.SIGNATURES[name]), name


def test_a_model_without_an_engine_is_refused_with_what_is_built():
    import modules
    for name in ("ddpminv", "cyclediff"):
        for model in (None, types.SimpleNamespace(unet=None, device="cpu")):
            with pytest.raises(NotImplementedError, match="model.engine") as e:
                modules.load_inverter(name, model=model)
            msg = str(e.value)
            assert "etainv_ddpm_invert_steps" in msg and "npi, proxnpi" in msg and "edict" in msg and "regdiffinv" in msg
            assert "ddpminv, cyclediff" in msg and "simple, ptp, masactrl, pnp" in msg
    with pytest.raises(NotImplementedError, match="ddpminv, cyclediff") as e:
        modules.load_inverter("nti", model=None)
    assert "npi, proxnpi" in str(e.value) and "simple, ptp, masactrl, pnp" in str(e.value)


def test_registry():
    import modules
    from modules.inversion.ddpm_inversion import DDPMInversion
    assert {"ddpminv", "cyclediff"} <= set(modules.get_inversion_methods())
    assert modules._inverters["ddpminv"] is DDPMInversion
    cyc = modules._inverters["cyclediff"]
    assert isinstance(cyc, partial) and cyc.func is DDPMInversion and cyc.keywords == {"markovian_forward": True}
    # every other inverter keeps refusing the "ddpm" scheduler name: only this class builds it
    from modules.inversion.diffusion_inversion import DiffusionInversion
    with pytest.raises(NotImplementedError, match="ddpminv / cyclediff"):
        DiffusionInversion.create_schedulers(None, types.SimpleNamespace(scheduler=None), "ddpm", 5)


@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("max_rows", [1, 2, 4, 12, 128])
@pytest.mark.parametrize("S", [1, 5, 50])
def test_chunk_plan_covers_every_step_once(S, max_rows, guided):
    from etainv.plan import DDPM_MAX_CHUNK, plan_ddpm_chunks
    per_step = 2 if guided else 1
    if per_step > max_rows:
        with pytest.raises(ValueError, match="UNet rows"):
            plan_ddpm_chunks(S, max_rows, guided)
        return
    chunks = plan_ddpm_chunks(S, max_rows, guided)
    steps = [j for c in chunks for j in range(c.first, c.first + c.k)]
    assert steps == list(range(S))                                               # every step once, in order
    assert all(1 <= c.k <= DDPM_MAX_CHUNK and c.rows == c.k * per_step <= max_rows for c in chunks)
    assert len(chunks) == -(-S // min(max_rows // per_step, DDPM_MAX_CHUNK))     # no more calls than needed
    # whole images of a step stay together too
    for n_img in (2, 3):
        if n_img * per_step <= max_rows:
            cs = plan_ddpm_chunks(S, max_rows, guided, n_img)
            assert [j for c in cs for j in range(c.first, c.first + c.k)] == list(range(S))
            assert all(c.rows == c.k * per_step * n_img <= max_rows for c in cs)


def test_chunk_plan_examples():
    from etainv.plan import Chunk, ddpm_guided, plan_ddpm_chunks
    assert plan_ddpm_chunks(5, 4, True) == [Chunk(0, 2, 4), Chunk(2, 2, 4), Chunk(4, 1, 2)]          # a max_img = 1 engine: 3 calls for 5 steps
    assert plan_ddpm_chunks(5, 4, False) == [Chunk(0, 4, 4), Chunk(4, 1, 1)]
    assert plan_ddpm_chunks(50, 128, True) == [Chunk(0, 50, 100)]
    assert plan_ddpm_chunks(50, 12, True, 3) == [Chunk(f, 2, 12) for f in range(0, 50, 2)]
    assert plan_ddpm_chunks(300, 1024, False) == [Chunk(0, 128, 128), Chunk(128, 128, 128), Chunk(256, 44, 44)]   # the launch's table holds 128 steps
    assert [ddpm_guided(g) for g in (0, 1, 1.0, 3.5, 9)] == [False, False, False, True, True]
    with pytest.raises(ValueError):
        plan_ddpm_chunks(0, 4, True)


def test_unet_rows_against_hand_counts():
    from etainv.flops import ddpm_unet_rows
    # S = 5, one step skipped: inversion 5 steps x 2 rows, backward 4 steps x 2 prompts x 2 rows
    assert ddpm_unet_rows(5, 1, 1, 2) == 10 + 16
    assert ddpm_unet_rows(5, 1, 1, 2, g_fwd=1) == 5 + 16                         # the simple editor inverts at guidance 1: the cond half alone
    assert ddpm_unet_rows(5, 1, 3, 2, g_fwd=1) == 3 * (5 + 16)
    assert ddpm_unet_rows(50, 18, 1, 2) == 100 + 32 * 4                          # the defaults: int(0.36 * 50) = 18 skipped
    assert ddpm_unet_rows(50, 18, 1, 1) == 100 + 32 * 2
    assert ddpm_unet_rows(2, 0, 1, 2) == 4 + 8                                   # a skip of 0 skips nothing


def test_host_coefficients_match_the_restatement():
    import numpy as np
    from etainv import pipeline as pl
    from tests import ddpminv_ref as dr
    ac = pl.alphas_cumprod()
    for S in (1, 5, 50):
        assert pl.ddpm_timesteps(S).tolist() == dr.timesteps(S)[::-1].tolist()
        for markov in (False, True):
            np.testing.assert_array_equal(pl.ddpm_sample_coefficients(ac, S, markov), dr.sample_coefficients(S, markov))
        for t in dr.timesteps(S):
            got, want = pl.ddpm_step_coefficients(ac, ac[0], S, t), dr.step_coefficients(S, t)
            np.testing.assert_allclose(got, want, rtol=1e-15, atol=0)
            assert (got[4] == 0) == (t == 0)                                     # sigma is exactly 0 at t = 0 and nowhere else
