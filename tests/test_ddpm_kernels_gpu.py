"""The three entry points of csrc/ddpm.hip against tests/ddpminv_ref.py in float64, their invariances bit for bit, and their refusals.

Bounds.  tests/golden/ddpm_inverse.npz holds, per (S, L, mode), how far the reference implementation's own float32 run lies from its float64 run
on the inputs of ddpminv_ref.kernel_case (relative L2 of the noised latents, the noise maps and the corrected latents).  A kernel result may lie
MULTIPLE = 4 times as far from float64: the kernel and the float32 reference evaluate the same expressions, but with differently rounded
coefficients (float64 rounded once against fp32 arithmetic) and, in the backward step, with contraction -- two fp32 evaluations of one
expression can fall on opposite sides of the float64 value, so their distances add (a factor 2) -- and the fixture's figure is one tensor's
sample, while the tests also run other images and seeds (the other factor 2).  The backward step has the form of the corrected latent
(x0 prediction, mean, + sigma z) and takes that yardstick, on the kernel's own guided noise; the guided noise itself is held, per element, to
the three roundings of u + g (c - u): the difference's error times g, the product's, the sum's, |err| <= 2^-24 (2 |g| |c - u| + |result|).

Measured on MI355X (this file's own printouts): see DESIGN.md, "DDPM inversion"."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import ddpminv_ref as dr

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
MULTIPLE = 4
EPS32 = 2.0 ** -24
MODES = {"ddpminv": False, "cyclediff": True}
SHAPES = [(l, n_img, S) for l in (8, 16, 24) for n_img in (1, 3) for S in (1, 5)]


@pytest.fixture(scope="module")
def lib():
    from etainv import _capi
    return _capi.load()


@pytest.fixture(scope="module")
def yard():
    return np.load(ROOT / "tests" / "golden" / "ddpm_inverse.npz")


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def cuda(v):
    return torch.from_numpy(np.array(v, dtype=np.float32, order="C")).cuda()      # (a copy: a reversed view has negative strides)


def case(S, L, n_img):
    """x0 (n,4,L,L), noise (S,n,4,L,L), eps (S,n,4,L,L): image 0 is the fixture's input"""
    parts = [dr.kernel_case(S, L, i) for i in range(n_img)]
    return tuple(np.concatenate([p[k] for p in parts], axis=int(k > 0)) for k in range(3))


def sample(lib, x0, noise, S, markov):
    from etainv import pipeline as pl
    return pl.ddpm_sample_latents(lib, cuda(x0), cuda(noise), dr.sample_coefficients(S, markov), markov)


def invert(lib, xts, first, k, eps_u, eps_c, g, S, want_eps=True):
    """steps [first, first + k) in xts order; eps given in xts order too -> (z, x, eps_out) (k,n,4,L,L)"""
    from etainv import pipeline as pl
    coef = np.stack([dr.step_coefficients(S, t) for t in dr.timesteps(S)[::-1]])[first:first + k]
    z, x, e = (torch.full_like(eps_c, float("nan")) for _ in range(3))
    pl.ddpm_invert_steps(lib, xts, first, k, eps_u, eps_c, g, coef, z, x, e if want_eps else None)
    return z, x, e


@pytest.mark.parametrize("tag", list(MODES))
@pytest.mark.parametrize("l,n_img,S", SHAPES)
def test_sample_latents(lib, yard, l, n_img, S, tag):
    x0, noise, _ = case(S, l, n_img)
    np.testing.assert_array_equal(np.concatenate([x0[0].ravel()[:4], noise[:, 0].ravel()[:4]]), yard[f"S{S}_L{l}/probe"][:8])
    xts = sample(lib, x0, noise, S, MODES[tag])
    torch.cuda.synchronize()
    assert xts.shape == (S + 1, n_img, 4, l, l) and torch.equal(xts[S].cpu(), torch.from_numpy(x0))
    want = dr.sample_latents(x0, noise, S, MODES[tag])
    bound = MULTIPLE * float(yard[f"S{S}_L{l}/{tag}/err_xts"])
    e0, e_all = rel(xts[:-1, 0].cpu(), want[:-1, 0]), rel(xts[:-1].cpu(), want[:-1])
    print(f"sample_latents {tag} l={l} n_img={n_img} S={S}: rel L2 vs float64 image 0 {e0:.3e}, all {e_all:.3e} (bound {bound:.3e})")
    assert e0 <= bound and e_all <= bound
    # an image's result does not depend on n_img or on its position
    for i in range(n_img):
        one = sample(lib, x0[i:i + 1], noise[:, i:i + 1], S, MODES[tag])
        assert torch.equal(one[:, 0], xts[:, i])


@pytest.mark.parametrize("tag", list(MODES))
@pytest.mark.parametrize("l,n_img,S", SHAPES)
def test_invert_steps(lib, yard, l, n_img, S, tag):
    x0, noise, eps = case(S, l, n_img)
    xts_np = dr.sample_latents(x0, noise, S, MODES[tag], dtype=np.float32)         # fp32 inputs of the step, as in the fixture
    xts, eps_x = cuda(xts_np), cuda(eps[::-1])                                      # (the kernel's step order is that of xts: descending t)
    z, x, e = invert(lib, xts, 0, S, None, eps_x, 1.0, S)
    torch.cuda.synchronize()
    assert torch.equal(e, eps_x) and torch.isfinite(z).all() and torch.isfinite(x).all()
    ts = dr.timesteps(S)[::-1]
    want = [dr.inverse_step(xts_np[j], xts_np[j + 1], eps[S - 1 - j], dr.step_coefficients(S, ts[j])) for j in range(S)]
    key5 = f"S5_L{l}/{tag}"
    # sigma == 0 (t = 0, the last index): z is exactly 0 and the corrected latent is mu
    assert ts[S - 1] == 0 and not z[S - 1].any()
    e_mu = rel(x[S - 1].cpu(), want[S - 1][2])
    print(f"invert_steps {tag} l={l} n_img={n_img} S={S}: sigma == 0 step, latent vs float64 mu {e_mu:.3e} (bound {MULTIPLE * float(yard[key5 + '/err_prev']):.3e})")
    assert e_mu <= MULTIPLE * float(yard[f"{key5}/err_prev"])
    if S > 1:
        zw, xw = np.stack([w[0] for w in want[:-1]]), np.stack([w[1] for w in want[:-1]])
        bz, bx = MULTIPLE * float(yard[f"{key5}/err_z"]), MULTIPLE * float(yard[f"{key5}/err_prev"])
        ez0, ex0 = rel(z[:-1, 0].cpu(), zw[:, 0]), rel(x[:-1, 0].cpu(), xw[:, 0])
        ez, ex = rel(z[:-1].cpu(), zw), rel(x[:-1].cpu(), xw)
        print(f"invert_steps {tag} l={l} n_img={n_img} S={S}: noise maps rel L2 vs float64 image 0 {ez0:.3e}, all {ez:.3e} (bound {bz:.3e}); "
              f"corrected latents {ex0:.3e}, {ex:.3e} (bound {bx:.3e})")
        assert max(ez0, ez) <= bz and max(ex0, ex) <= bx
    # k = S in one launch == k = 1 step by step, bit for bit; so is a chunk that starts in the middle
    for j in range(S):
        z1, x1, e1 = invert(lib, xts, j, 1, None, eps_x[j:j + 1], 1.0, S)
        assert torch.equal(z1[0], z[j]) and torch.equal(x1[0], x[j]) and torch.equal(e1[0], e[j])
    if S > 2:
        z2, x2, _ = invert(lib, xts, 2, 2, None, eps_x[2:4], 1.0, S, want_eps=False)
        assert torch.equal(z2, z[2:4]) and torch.equal(x2, x[2:4])
    # n_img images == n_img one-image calls
    for i in range(n_img):
        zi, xi, _ = invert(lib, xts[:, i:i + 1].contiguous(), 0, S, None, eps_x[:, i:i + 1].contiguous(), 1.0, S)
        assert torch.equal(zi[:, 0], z[:, i]) and torch.equal(xi[:, 0], x[:, i])


@pytest.mark.parametrize("l,n_img,S", [(8, 1, 1), (16, 3, 5), (24, 1, 5)])
def test_invert_steps_guided(lib, l, n_img, S):
    """with eps_u: the guided noise is u + g (c - u) in three roundings, and the rest is the unguided launch on it, bit for bit"""
    x0, noise, eps = case(S, l, n_img)
    g = 3.5
    u_np = np.random.default_rng(5 + l).standard_normal(eps.shape).astype(np.float32)
    xts = cuda(dr.sample_latents(x0, noise, S, False, dtype=np.float32))
    u, c = cuda(u_np), cuda(eps)
    z, x, e = invert(lib, xts, 0, S, u, c, g, S)
    want = dr.cfg(u_np.astype(np.float64), eps.astype(np.float64), g)
    tol = 1.01 * EPS32 * (2 * g * np.abs(eps.astype(np.float64) - u_np) + np.abs(want))
    err = np.abs(e.cpu().numpy() - want)
    print(f"invert_steps guided l={l} n_img={n_img} S={S}: guided noise max |err| / bound {float((err / tol).max()):.3f}")
    assert (err <= tol).all()
    z2, x2, e2 = invert(lib, xts, 0, S, None, e, 1.0, S)
    assert torch.equal(z2, z) and torch.equal(x2, x) and torch.equal(e2, e)
    z3, x3, _ = invert(lib, xts, 0, S, u, c, g, S, want_eps=False)                    # the guided noise is an optional output
    assert torch.equal(z3, z) and torch.equal(x3, x)


@pytest.mark.parametrize("t", [600, 0])
@pytest.mark.parametrize("l,n_img,n_prompts", [(8, 1, 1), (8, 3, 2), (16, 1, 2), (16, 3, 4), (24, 1, 4), (24, 3, 2)])
def test_backward_step(lib, yard, l, n_img, n_prompts, t):
    from etainv import _capi
    from etainv import pipeline as pl
    S, scales = 5, [3.5, 9.0, 1.0, 0.0][:n_prompts]
    ac = dr.alphas_cumprod()
    a_t, a_p, var = float(ac[t]), float(dr.alpha_prev(ac, t, S)), float(dr.variance(ac, t, S))
    assert (var == 0) == (t == 0)
    rng = np.random.default_rng(100 * l + 10 * n_img + n_prompts)
    rows = n_prompts * n_img
    x_np, u_np, c_np = (rng.standard_normal((rows, 4, l, l)).astype(np.float32) for _ in range(3))
    z_np = rng.standard_normal((n_img, 4, l, l)).astype(np.float32)
    x, u, c, z = cuda(x_np), cuda(u_np), cuda(c_np), cuda(z_np)
    out, eps = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    pl.ddpm_backward_step(lib, x, u, c, scales, z, a_t, a_p, var, out, eps)
    # bit-equal to etainv_cfg_combine per prompt followed by etainv_ddim_eta_step(eta = 1, noise = z) per image
    st, n = _capi.stream_ptr(), n_img * 4 * l * l
    eps2, out2 = torch.empty_like(x), torch.empty_like(x)
    for p in range(n_prompts):
        sl = slice(p * n_img, (p + 1) * n_img)
        _capi.check(lib.etainv_cfg_combine(_capi.ptr(u[sl]), _capi.ptr(c[sl]), scales[p], _capi.ptr(eps2[sl]), n, _capi.F32, st))
        for i in range(n_img):
            r = p * n_img + i
            _capi.check(lib.etainv_ddim_eta_step(_capi.ptr(x[r]), _capi.ptr(eps2[r]), 1.0, None, 0, _capi.ptr(z[i]), a_t, a_p, var, 1, 4, l * l,
                                                 _capi.ptr(out2[r]), _capi.F32, st))
    torch.cuda.synchronize()
    assert torch.equal(eps, eps2) and torch.equal(out, out2)
    out3 = torch.empty_like(x)
    pl.ddpm_backward_step(lib, x, u, c, scales, z, a_t, a_p, var, out3, None)        # the guided noise is an optional output
    assert torch.equal(out3, out)
    # against float64: the guided noise per element, the step on that noise at the corrected latent's yardstick
    g = np.repeat(np.asarray(scales, dtype=np.float64), n_img).reshape(-1, 1, 1, 1)
    want_eps = dr.cfg(u_np.astype(np.float64), c_np.astype(np.float64), g)
    tol = 1.01 * EPS32 * (2 * np.abs(g) * np.abs(c_np.astype(np.float64) - u_np) + np.abs(want_eps))
    assert (np.abs(eps.cpu().numpy() - want_eps) <= tol).all()
    want = dr.ddim_eta1_step(x_np.astype(np.float64), eps.cpu().double().numpy(), np.concatenate([z_np] * n_prompts).astype(np.float64), a_t, a_p, var)
    e, bound = rel(out.cpu(), want), MULTIPLE * float(yard[f"S5_L{l}/ddpminv/err_prev"])
    print(f"backward_step l={l} n_img={n_img} prompts={n_prompts} t={t}: rel L2 vs float64 {e:.3e} (bound {bound:.3e})")
    assert e <= bound and torch.isfinite(out).all()
    # rows of one image under other prompt counts / positions: an element's result depends on its own inputs only
    one = torch.empty(1, 4, l, l, device="cuda")
    r = rows - 1
    pl.ddpm_backward_step(lib, x[r:r + 1].contiguous(), u[r:r + 1].contiguous(), c[r:r + 1].contiguous(), scales[-1:], z[n_img - 1:n_img].contiguous(),
                          a_t, a_p, var, one, None)
    assert torch.equal(one[0], out[r])


def test_refusals(lib):
    """every refusal of the three entry points: non-zero status, a message, nothing written"""
    from etainv import _capi
    l, S, n = 8, 3, 2
    f = lambda *shape: torch.zeros(*shape, 4, l, l, device="cuda")
    x0, noise, xts = f(n), f(S, n), f(S + 1, n)
    eps, z, xo = f(S, n), f(S, n), f(S, n)
    ab, coef = (C.c_double * (2 * 300))(*([0.5] * 600)), (C.c_double * (5 * 200))(*([0.5] * 1000))
    scales = (C.c_float * 4)(1.0, 2.0, 3.0, 4.0)
    p, st = _capi.ptr, _capi.stream_ptr()
    nan, inf = float("nan"), float("inf")

    def refused(status, what):
        msg = lib.etainv_last_error().decode()
        assert status != 0 and what in msg, (status, what, msg)

    sample = lambda x0_=p(x0), noise_=p(noise), ab_=ab, markov=0, xts_=p(xts), S_=S, n_=n, l_=l: \
        lib.etainv_ddpm_sample_latents(x0_, noise_, ab_, markov, xts_, S_, n_, l_, st)
    assert sample() == 0
    for kw in (dict(x0_=None), dict(noise_=None), dict(ab_=None), dict(xts_=None)):
        refused(sample(**kw), "null pointer")
    for bad in (7, 97, 0, -8):
        refused(sample(l_=bad), "latent side")
    refused(sample(S_=0), "at least 1")
    refused(sample(n_=0), "at least 1")
    refused(sample(S_=257), "ETAINV_DDPM_MAX_STEPS")
    refused(sample(markov=2), "markovian")
    refused(sample(x0_=p(x0) + 4), "aligned")
    refused(sample(ab_=(C.c_double * 6)(0.5, 0.5, nan, 0.5, 0.5, 0.5)), "non-finite")

    invert = lambda xts_=p(xts), S_=S, first=0, k=S, u=None, c=p(eps), g=1.0, coef_=coef, z_=p(z), xo_=p(xo), eo=None, n_=n, l_=l: \
        lib.etainv_ddpm_invert_steps(xts_, S_, first, k, u, c, g, coef_, z_, xo_, eo, n_, l_, st)
    assert invert() == 0 and invert(u=p(eps), eo=p(f(S, n))) == 0
    for kw in (dict(xts_=None), dict(c=None), dict(coef_=None), dict(z_=None), dict(xo_=None)):
        refused(invert(**kw), "null pointer")
    for bad in (7, 97):
        refused(invert(l_=bad), "latent side")
    for kw in (dict(S_=0), dict(k=0), dict(n_=0), dict(k=-1)):
        refused(invert(**kw), "at least 1")
    refused(invert(S_=200, k=129), "ETAINV_DDPM_MAX_CHUNK")
    for kw in (dict(first=-1), dict(first=1), dict(first=S, k=1), dict(k=S + 1)):
        refused(invert(**kw), "inside")
    for bad in (nan, inf, -inf):
        refused(invert(u=p(eps), g=bad), "finite")
    refused(invert(coef_=(C.c_double * 15)(*([0.5] * 7 + [inf] + [0.5] * 7))), "non-finite")
    refused(invert(coef_=(C.c_double * 15)(*([0.5, 0.0, 0.5, 0.5, 0.5] * 3))), "positive")
    refused(invert(z_=p(z) + 8), "aligned")

    rows = 2 * n
    x, u, c, out = f(rows), f(rows), f(rows), f(rows)
    zz = f(n)
    back = lambda x_=p(x), u_=p(u), c_=p(c), g_=scales, np_=2, z_=p(zz), a_t=0.5, a_p=0.6, var=0.1, out_=p(out), eo=None, n_=n, l_=l: \
        lib.etainv_ddpm_backward_step(x_, u_, c_, g_, np_, z_, a_t, a_p, var, out_, eo, n_, l_, st)
    assert back() == 0
    for kw in (dict(x_=None), dict(u_=None), dict(c_=None), dict(g_=None), dict(z_=None), dict(out_=None)):
        refused(back(**kw), "null pointer")
    for bad in (7, 97):
        refused(back(l_=bad), "latent side")
    refused(back(n_=0), "at least 1")
    for bad in (0, 5, -1):
        refused(back(np_=bad), "n_prompts")
    for bad in (nan, inf):
        refused(back(g_=(C.c_float * 4)(1.0, bad, 3.0, 4.0)), "finite")
    assert back(np_=1, g_=(C.c_float * 4)(1.0, nan, 3.0, 4.0), n_=n) == 0                 # (only the scales in use are read)
    for kw in (dict(a_t=0.0), dict(a_t=1.0), dict(a_p=0.0), dict(a_p=1.5), dict(a_t=nan)):
        refused(back(**kw), "alphas_cumprod")
    for bad in (nan, -0.1, inf):
        refused(back(var=bad), "variance")
    refused(back(out_=p(out) + 4), "aligned")
    out.fill_(7.0)                                                                        # a refused call launches nothing
    refused(back(np_=5), "n_prompts")
    torch.cuda.synchronize()
    assert (out == 7.0).all()
