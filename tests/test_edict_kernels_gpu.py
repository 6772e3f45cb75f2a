"""The three EDICT step kernels (csrc/step_kernels.hip: etainv_edict_couple, etainv_edict_mix, etainv_edict_couple_mix) against float64.

Bound.  Every comparison allows what the number formats allow and nothing else.  The kernels compute in fp32 with one rounding per
operation (each product-sum is an explicit fmaf), so the error of a result follows from its expression: `_V` below carries, for every
intermediate, its float64 value, a bound `mag` of its magnitude (the sum of the absolute terms) and a bound `err` of its distance from
the float64 value; an operation adds U32 * mag (U32 = 2^-24, half an fp32 ulp relative) to the propagated errors of its operands, and the
store adds one rounding of the output dtype (half an ulp relative, or half the subnormal spacing where the result is that small: about 25
of 2^19 results land below fp16's 6e-5).  Counted per expression, with T the sum of the absolute terms:
  couple     eps = fma(g, c - u, u); v = fma(b, eps, a * base)      k = 4 operations (2 without guidance):  err <= k U32 T
  mix        x' = fma(p, x, q y); y' = fma(p, y, q x')               k = 2 each, y' inherits q * err(x')
  un-mix     y' = fma(-q, x, y) / p; x' = fma(-q, y', x) / p         k = 2 each, every term divided by p, x' inherits q / p * err(y')
  couple_mix = couple, then mix on its unrounded result
q is the kernel's fp32 `1 - p` (exact for p >= 0.5).  The scalars g, a, b, p are fp32 values, so they carry no error of their own.
Second-order terms (u^2) are covered by a factor 1.001 on the whole bound."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
U_OUT = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
SUB_OUT = {torch.float32: 2.0 ** -150, torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134}   # half the spacing of the subnormals
SIZES = [1, 255, 256 * 2048 + 77]            # below a block, a ragged block, one past the grid cap (2048 blocks of 256 threads)
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
f32 = lambda v: float(np.float32(v))


class _V:
    def __init__(self, val, mag=None, err=None):
        self.val = np.asarray(val, dtype=np.float64)
        self.mag = np.abs(self.val) if mag is None else mag
        self.err = np.zeros_like(self.val) if err is None else err

    def _op(self, val, mag, err):
        return _V(val, mag, err + U32 * mag)

    def sub(self, o):
        return self._op(self.val - o.val, self.mag + o.mag, self.err + o.err)

    def scale(self, s):
        return self._op(s * self.val, abs(s) * self.mag, abs(s) * self.err)

    def fma(self, s, addend):                                       # s * self + addend, one rounding
        return self._op(s * self.val + addend.val, abs(s) * self.mag + addend.mag, abs(s) * self.err + addend.err)

    def div(self, s):
        return self._op(self.val / s, self.mag / abs(s), self.err / abs(s))

    def stored(self, dtype):                                        # the rounding of the store, and what a later kernel reads back
        err = self.err + np.maximum(U_OUT[dtype] * (np.abs(self.val) + self.err), SUB_OUT[dtype])
        return _V(self.val, np.abs(self.val) + err, err)

    def bound(self):
        return 1.001 * self.err


def v_couple(base, u, c, g, a, b):
    eps = c if u is None else c.sub(u).fma(g, u)
    return eps.fma(b, base.scale(a))


def v_mix(x, y, p, inverse):
    q = float(np.float32(1) - np.float32(p))
    if inverse:
        y = x.fma(-q, y).div(p)
        x = y.fma(-q, x).div(p)
    else:
        x = x.fma(p, y.scale(q))
        y = y.fma(p, x.scale(q))
    return x, y


def _draw(n, dtype, seed, k):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g).to(dtype).cuda() for _ in range(k)]


V = lambda t: _V(t.double().cpu().numpy())


def _check(got, v, dtype, what):
    v = v.stored(dtype)
    diff = np.abs(got.double().cpu().numpy() - v.val)
    worst = float((diff / np.maximum(v.bound(), 1e-300)).max())
    print(f"{what}: max |diff| {diff.max():.3e}, worst diff / bound {worst:.3f}")
    assert worst <= 1.0, what


@pytest.fixture(scope="module")
def lib():
    from etainv import _capi
    return _capi.load()


def couple(lib, base, u, c, g, a, b, out):
    from etainv import _capi
    _capi.check(lib.etainv_edict_couple(_capi.ptr(base), _capi.ptr(u), _capi.ptr(c), g, a, b, _capi.ptr(out), base.numel(),
                                        _capi.dtype_code(base.dtype), _capi.stream_ptr()))


def mix(lib, x, y, p, inverse):
    from etainv import _capi
    _capi.check(lib.etainv_edict_mix(_capi.ptr(x), _capi.ptr(y), p, inverse, x.numel(), _capi.dtype_code(x.dtype), _capi.stream_ptr()))


def couple_mix(lib, x, y, base_is_y, u, c, g, a, b, p):
    from etainv import _capi
    _capi.check(lib.etainv_edict_couple_mix(_capi.ptr(x), _capi.ptr(y), base_is_y, _capi.ptr(u), _capi.ptr(c), g, a, b, p, x.numel(),
                                            _capi.dtype_code(x.dtype), _capi.stream_ptr()))


G, A, B_, P = f32(3.0), f32(1.0507), f32(-0.1103), f32(0.93)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("in_place", [False, True])
def test_couple(lib, n, dtype, guided, in_place):
    base, u, c = _draw(n, dtype, 10 + n % 7, 3)
    u = u if guided else None
    want = v_couple(V(base), None if u is None else V(u), V(c), G, A, B_)
    keep = [t.clone() for t in (u, c) if t is not None]
    out = base if in_place else torch.full_like(base, float("nan"))
    before = base.clone()
    couple(lib, base, u, c, G, A, B_, out)
    torch.cuda.synchronize()
    _check(out, want, dtype, f"couple n={n} {dtype} guided={guided} in_place={in_place}")
    assert in_place or torch.equal(base, before)
    assert all(torch.equal(a, b) for a, b in zip(keep, [t for t in (u, c) if t is not None]))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("p", [P, f32(0.3), 1.0])
def test_mix(lib, n, dtype, inverse, p):
    x, y = _draw(n, dtype, 20 + n % 5, 2)
    wx, wy = v_mix(V(x), V(y), p, inverse)
    mix(lib, x, y, p, inverse)
    torch.cuda.synchronize()
    _check(x, wx, dtype, f"mix x n={n} {dtype} inverse={inverse} p={p}")
    _check(y, wy, dtype, f"mix y n={n} {dtype} inverse={inverse} p={p}")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("base_is_y", [0, 1])
def test_couple_mix(lib, n, dtype, guided, base_is_y):
    x, y, u, c = _draw(n, dtype, 30 + n % 3, 4)
    u = u if guided else None
    vx, vy = V(x), V(y)
    v = v_couple(vy if base_is_y else vx, None if u is None else V(u), V(c), G, A, B_)
    wx, wy = v_mix(vx if base_is_y else v, v if base_is_y else vy, P, 0)
    couple_mix(lib, x, y, base_is_y, u, c, G, A, B_, P)
    torch.cuda.synchronize()
    _check(x, wx, dtype, f"couple_mix x n={n} {dtype} guided={guided} base_is_y={base_is_y}")
    _check(y, wy, dtype, f"couple_mix y n={n} {dtype} guided={guided} base_is_y={base_is_y}")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("base_is_y", [0, 1])
def test_couple_mix_is_couple_then_mix_bit_for_bit(lib, n, guided, base_is_y):
    x, y, u, c = _draw(n, torch.float32, 40, 4)
    u = u if guided else None
    x2, y2 = x.clone(), y.clone()
    couple_mix(lib, x, y, base_is_y, u, c, G, A, B_, P)
    base = y2 if base_is_y else x2
    couple(lib, base, u, c, G, A, B_, base)
    mix(lib, x2, y2, P, 0)
    torch.cuda.synchronize()
    assert torch.equal(x, x2) and torch.equal(y, y2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("S,t", [(50, 501), (3, 666), (4, 750)])
def test_inversion_step_then_denoising_step_returns_base(lib, dtype, S, t):
    """x1 = q x0 + b_i eps, then x0' = x1 / q + b_d eps with the host's fp32 coefficients of one timestep and the same eps.  |x0' - x0| is
    bounded by the kernels' rounding through both steps (1/q amplifies the first step's) plus what the fp32 coefficients themselves miss the
    identity by, |a_d a_i - 1| |x0| + |a_d b_i + b_d| |eps|, evaluated in float64 from the coefficient values."""
    from etainv.pipeline import alphas_cumprod, edict_coefficients
    ac = torch.as_tensor(alphas_cumprod().astype(np.float32))
    (a_i, b_i), (a_d, b_d) = edict_coefficients(ac, ac[0], t, S, True), edict_coefficients(ac, ac[0], t, S, False)
    x0, u, c = _draw(SIZES[2], dtype, 50, 3)
    vu, vc = V(u), V(c)
    v1 = v_couple(V(x0), vu, vc, G, a_i, b_i).stored(dtype)
    v2 = v_couple(v1, vu, vc, G, a_d, b_d).stored(dtype)
    eps = vu.val + G * (vc.val - vu.val)
    coef = abs(a_d * a_i - 1.0) * np.abs(V(x0).val) + abs(a_d * b_i + b_d) * np.abs(eps)
    x = x0.clone()
    couple(lib, x, u, c, G, a_i, b_i, x)
    couple(lib, x, u, c, G, a_d, b_d, x)
    torch.cuda.synchronize()
    diff = np.abs(x.double().cpu().numpy() - V(x0).val)
    worst = float((diff / (v2.bound() + coef)).max())
    print(f"couple round trip S={S} t={t} {dtype}: 1/q = {a_d:.3f}, max |diff| {diff.max():.3e}, worst diff / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("p", [P, 0.5])
def test_mix_then_unmix_returns_the_pair(lib, dtype, p):
    """exact in real arithmetic (both directions use the same q = 1 - p); the bound is the rounding of the four expressions, the un-mix's 1/p
    included"""
    x0, y0 = _draw(SIZES[2], dtype, 60, 2)
    x1, y1 = v_mix(V(x0), V(y0), p, 0)
    x2, y2 = v_mix(x1.stored(dtype), y1.stored(dtype), p, 1)
    x, y = x0.clone(), y0.clone()
    mix(lib, x, y, p, 0)
    mix(lib, x, y, p, 1)
    torch.cuda.synchronize()
    for name, got, v, orig in (("x", x, x2, x0), ("y", y, y2, y0)):
        v = v.stored(dtype)
        chain = np.abs(v.val - V(orig).val)                                             # the float64 chain is the identity up to ITS rounding
        assert chain.max() < 1e-13
        diff = np.abs(got.double().cpu().numpy() - V(orig).val)
        worst = float((diff / (v.bound() + chain)).max())
        print(f"mix round trip {name} p={p} {dtype}: max |diff| {diff.max():.3e}, worst diff / bound {worst:.3f}")
        assert worst <= 1.0


def test_refusals_on_device_pointers(lib):
    from etainv import _capi
    x, y, c = _draw(64, torch.float32, 70, 3)
    st = _capi.stream_ptr()
    before = (x.clone(), y.clone())
    assert lib.etainv_edict_mix(_capi.ptr(x), _capi.ptr(y), 0.0, 0, 64, _capi.F32, st) != 0 and b"(0, 1]" in lib.etainv_last_error()
    assert lib.etainv_edict_mix(_capi.ptr(x), _capi.ptr(y), 1.25, 1, 64, _capi.F32, st) != 0 and b"(0, 1]" in lib.etainv_last_error()
    assert lib.etainv_edict_couple(_capi.ptr(x), None, None, 3.0, 1.0, 0.1, _capi.ptr(x), 64, _capi.F32, st) != 0 and b"null" in lib.etainv_last_error()
    assert lib.etainv_edict_couple_mix(_capi.ptr(x), _capi.ptr(x), 0, None, _capi.ptr(c), 3.0, 1.0, 0.1, 0.93, 64, _capi.F32, st) != 0
    assert b"pair" in lib.etainv_last_error()
    assert lib.etainv_edict_couple_mix(_capi.ptr(x), _capi.ptr(y), 0, None, _capi.ptr(c), 3.0, 1.0, 0.1, 0.93, 64, 5, st) != 0
    assert b"dtype" in lib.etainv_last_error()
    torch.cuda.synchronize()
    assert torch.equal(x, before[0]) and torch.equal(y, before[1])                          # a refused call launches nothing
