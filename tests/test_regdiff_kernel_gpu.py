"""etainv_noise_regularize (csrc/regularize.hip) per element against the float64 closed form of tests/regdiff_ref.py.

Input of every case: regdiff_ref.multiscale_field (white noise + 0.5 x nearest-upsampled white noise at factors 2, 4, 8, 16 + 0.05), on which
every pyramid level matters (tests/test_regdiff_ref.py::test_every_level_matters_on_the_kernel_input).  Bound per image: 8 x the max-abs
deviation of the fp32 autograd restatement from float64 on the same image, computed here on the CPU -- the kernel has that restatement's
arithmetic with other reduction trees and contraction.  Sizes: 8 (one level), 16 (two), 20 (20, 10, 5: an odd level), 44 (44, 22, 11, 5),
64 (the largest with level 0 in LDS), 96 (five levels, level 0 in eps_out); every size at n_img 1 and 3.

Measured on MI355X (this file's own printouts): see DESIGN.md, "Regularised DDIM inversion"."""
import numpy as np
import pytest
import torch

from tests import regdiff_ref as rr

pytestmark = pytest.mark.gpu


def run(eps_c, shifts, eps_u=None, g=1.0, x=None, a_from=1.0, a_to=1.0, out=None, **params):
    """one call of the entry point on device tensors; returns (eps_out, x_out)"""
    from etainv import _capi
    lib = _capi.load()
    kw = {**rr.DEFAULTS, **params}
    n, _, L, _ = eps_c.shape
    out = torch.empty_like(eps_c) if out is None else out
    x_out = torch.empty_like(x) if x is not None else None
    sh = torch.from_numpy(np.ascontiguousarray(shifts)).cuda() if shifts is not None and np.size(shifts) else None
    _capi.check(lib.etainv_noise_regularize(_capi.ptr(eps_u), _capi.ptr(eps_c), float(g), _capi.ptr(out), _capi.ptr(x), float(a_from), float(a_to),
                                            _capi.ptr(x_out), n, L, _capi.ptr(sh), kw["num_reg_steps"], kw["num_ac_rolls"], kw["lambda_ac"],
                                            kw["lambda_kl"], _capi.stream_ptr()))
    torch.cuda.synchronize()
    return out, x_out


def check(got, case, images, what):
    """per image: max |kernel - float64| against that image's bound; prints the ratio observed / fp32-restatement deviation"""
    got = got.double().cpu().numpy()
    assert np.isfinite(case["bound"]).all() and (case["bound"] > 0).all()
    for k, img in enumerate(images):
        err = np.abs(got[k] - case["ref"][img]).max()
        print(f"{what} image {img}: max-abs error {err:.3e}, fp32 restatement {case['dev32'][img]:.3e}, ratio {err / case['dev32'][img]:.2f} (bound 8)")
        assert err <= case["bound"][img], (what, img, err, case["bound"][img])


@pytest.mark.parametrize("n_img", [1, 3])
@pytest.mark.parametrize("L", rr.KERNEL_SIZES)
def test_regularize_vs_float64(L, n_img):
    case = rr.kernel_case(L)
    out, _ = run(case["x"][:n_img].cuda(), case["shifts"])
    check(out, case, range(n_img), f"L = {L} n_img = {n_img}")


@pytest.mark.parametrize("L,params", [(20, dict(lambda_ac=0.0)), (20, dict(lambda_kl=0.0)), (96, dict(lambda_kl=0.0)), (44, dict(num_ac_rolls=1)),
                                      (64, dict(num_reg_steps=2, num_ac_rolls=3, lambda_ac=7.0, lambda_kl=3.0))])
def test_parameter_settings(L, params):
    """one loss alone, a single roll per round (the shift table then has num_reg_steps rows), other counts and weights.  (num_ac_rolls = 1
    takes the whole lambda_ac in one step and diverges on some inputs at small sizes, in the reference too: L = 44 converges on all three)"""
    case = rr.kernel_case(L, **params)
    out, _ = run(case["x"].cuda(), case["shifts"], **params)
    check(out, case, range(3), f"L = {L} {params}")


@pytest.mark.parametrize("params", [dict(num_reg_steps=0), dict(lambda_ac=0.0, lambda_kl=0.0), dict(lambda_ac=-1.0, lambda_kl=-2.0)])
def test_pass_through(params):
    """no rounds, or no loss with a positive weight: the noise comes back bit for bit -- also the guided one, and the step still runs"""
    L = 20
    x = rr.kernel_case(L)["x"].cuda()
    out, _ = run(x, None, **params)
    assert torch.equal(out, x)
    u = x.flip(0).contiguous()
    lat = (0.5 * x + 0.1).contiguous()
    out, stepped = run(x, None, eps_u=u, g=1.625, x=lat, a_from=0.9, a_to=0.8, **params)
    guided = u + 1.625 * (x - u)
    assert torch.allclose(out, guided, rtol=0, atol=2e-6)                # two roundings of values below 16 (ulp 9.5e-7), contracted or not
    want = rr.ddim_inverse_step(lat.double().cpu().numpy(), out.double().cpu().numpy(), 0.9, 0.8)
    assert np.abs(stepped.double().cpu().numpy() - want).max() <= 2e-6    # six roundings, half an ulp (4.8e-7) each, of values below 8


_guided = {}


@pytest.mark.parametrize("L", [20, 64, 96])
@pytest.mark.parametrize("form", ["cfg", "step", "both"])
def test_fused_forms_vs_composed_reference(L, form):
    """CFG combine in front (g from the forward guidance table), DDIM inverse step behind, and both: against the float64 composition
    guidance -> closed form -> step.  Noise bound: 8 x the fp32 restatement's deviation on the guided input; latent bound: the step is
    x' = a x + b eps with |b| < 1 at these alphas, so the noise bound plus four fp32 roundings of values up to 8 (4 x 4.8e-7)."""
    t = 481
    g = rr.guidance(t)
    ac = rr.alphas_cumprod()
    a_from, a_to = float(ac[t - 20]), float(ac[t])
    base = rr.kernel_case(L)
    x3 = base["x"]
    if form == "step":
        eps_u, eps_c = None, x3
    else:
        gen = torch.Generator().manual_seed(7 + L)
        eps_u = (x3 + 0.3 * torch.randn(x3.shape, generator=gen)).contiguous()
        eps_c = x3
    lat = (0.8 * rr.multiscale_field(L, 3, seed=300 + L)).contiguous() if form != "cfg" else None
    if form == "step":
        ref, dev32 = base["ref"], base["dev32"]
    else:
        if L not in _guided:                                            # (shared by "cfg" and "both")
            guided64 = eps_u.double().numpy() + g * (eps_c.double().numpy() - eps_u.double().numpy())
            r = np.stack([rr.regularize_closed(v, base["shifts"]) for v in guided64])
            d = np.array([np.abs(rr.regularize_autograd(torch.from_numpy(v).float(), base["shifts"]).double().numpy() - w).max()
                          for v, w in zip(guided64, r)])
            _guided[L] = (r, d)
        ref, dev32 = _guided[L]
    out, stepped = run(eps_c.cuda(), base["shifts"], eps_u=None if eps_u is None else eps_u.cuda(), g=g,
                       x=None if lat is None else lat.cuda(), a_from=a_from, a_to=a_to)
    for i in range(3):
        err = np.abs(out[i].double().cpu().numpy() - ref[i]).max()
        print(f"L = {L} {form} image {i}: noise max-abs error {err:.3e}, fp32 restatement {dev32[i]:.3e}, ratio {err / dev32[i]:.2f} (bound 8)")
        assert err <= 8 * dev32[i]
        if lat is not None:
            want = rr.ddim_inverse_step(lat[i].double().numpy(), ref[i], a_from, a_to)
            e_x = np.abs(stepped[i].double().cpu().numpy() - want).max()
            print(f"L = {L} {form} image {i}: latent max-abs error {e_x:.3e}")
            assert e_x <= 8 * dev32[i] + 4 * 4.8e-7
    if form == "step":                                                  # the unfused call gives the same noise, bit for bit
        plain, _ = run(eps_c.cuda(), base["shifts"])
        assert torch.equal(plain, out)


@pytest.mark.parametrize("L", [20, 96])
def test_eps_out_may_alias_eps_c(L):
    """in place (L = 96: eps_out also is the published copy of level 0 that the neighbours read)"""
    case = rr.kernel_case(L)
    x = case["x"].cuda()
    want, _ = run(x, case["shifts"])
    buf = x.clone()
    out, _ = run(buf, case["shifts"], out=buf)
    assert out.data_ptr() == buf.data_ptr() and torch.equal(buf, want)


@pytest.mark.parametrize("L", [16, 44, 96])
def test_batch_of_three_equals_single_calls_and_repeats(L):
    """an image's result does not depend on n_img or on its position, and two identical calls agree bit for bit"""
    case = rr.kernel_case(L)
    x = case["x"].cuda()
    three, _ = run(x, case["shifts"])
    again, _ = run(x, case["shifts"])
    assert torch.equal(three, again)
    for i in range(3):
        one, _ = run(x[i:i + 1].contiguous(), case["shifts"])
        assert torch.equal(one[0], three[i]), i
    swapped, _ = run(x.flip(0).contiguous(), case["shifts"])
    assert torch.equal(swapped.flip(0), three)
