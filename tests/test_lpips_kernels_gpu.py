"""The LPIPS kernels of csrc/lpips.hip one by one on the device, in the three compute dtypes.

  preprocess   each value is the float64 result of tests/lpips_ref.preprocess rounded to the dtype, or its neighbour; the fourth channel is exactly 0
  conv2d_relu  the five AlexNet layer forms at the smallest sizes where each edge exists, n = 2 and 3 (M is no tile multiple), ReLU on and off, in
               two families: `exact` (small integers from tests/gemm_ref's hashes: every product and partial sum is an integer, bit for bit in any
               order) and `random` against the counted bound of tests/gemm_ref.py, e = gamma_l(K + 1 + 4) (sum |a||w| + |bias|),
               bound = U_RND (|ref| + e) + e + ABS_FLOOR (ReLU is 1-Lipschitz and maps 0 to 0: the bound carries over)
  maxpool3s2   bit for bit against F.max_pool2d of the same values, negative inputs included
  distance     against float64 torch on the same stored features: |s - s_64| <= 1e-12 * 4 max_c w_c (a tap's value cannot exceed 4 max w; the
               float64 error of fewer than 400 non-negative terms and the two norms is below 1e-13 of that), and the exact properties"""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import lpips_ref as lr
from tests.gemm_ref import ABS_FLOOR, DTYPES3, NAME, U_RND, exact_w_density, gamma_l, hash_int, hash_ternary, worst

pytestmark = pytest.mark.gpu
name_of = lambda dt: NAME[dt]
INT = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}


def _lib():
    from etainv import _capi
    return _capi, _capi.load()


def _ordered(t):
    """the values' bit patterns as integers that ascend with the value (sign-magnitude -> two's complement)"""
    b = t.contiguous().view(INT[t.dtype]).to(torch.int64)
    top = 1 << (8 * t.element_size() - 1)
    return torch.where(b >= 0, b, -(b & (top - 1)))


# ---------------------------------------------------------------------------------------------------------------- preprocess
@pytest.mark.parametrize("dtype", DTYPES3, ids=name_of)
@pytest.mark.parametrize("size", [(31, 31), (35, 38)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mask_kind", ["none", "one", "per-pair"])
@pytest.mark.parametrize("rng", [(-1.0, 1.0), (0.0, 1.0), (0.0, 255.0)], ids=lambda r: f"{r[0]:g}..{r[1]:g}")
def test_preprocess(rng, mask_kind, size, dtype):
    from metrics.lpips import lpips_preprocess
    (lo, hi), (h, w), b = rng, size, 2
    g = torch.Generator().manual_seed(h * 1000 + w + int(hi))
    x = (lo + (hi - lo) * torch.rand(2 * b, 3, h, w, generator=g)).float()
    if hi == 255.0:
        x = x.round()
    mask = None
    if mask_kind != "none":
        mask = (torch.rand(1 if mask_kind == "one" else b, h, w, generator=g) > 0.6).float()
        mask[:, ::3, 1::4] = 0.375                                                   # a fractional mask
    got = lpips_preprocess(x.cuda(), (lo, hi), None if mask is None else mask.cuda(), dtype)
    assert got.shape == (2 * b, h, w, 4) and got.dtype == dtype and got.is_contiguous()
    got = got.cpu()
    assert bool((got[..., 3].contiguous().view(INT[dtype]) == 0).all())                  # exactly +0
    want = lr.preprocess(x, lo, hi, mask).permute(0, 2, 3, 1).contiguous()
    off = (_ordered(got[..., :3]) - _ordered(want.to(dtype))).abs()
    print(f"lpips-preprocess {name_of(dtype)} {lo:g}..{hi:g} {mask_kind} {h}x{w}: {int((off == 1).sum())} of {off.numel()} values are the neighbour")
    assert int(off.max()) <= 1
    if mask is not None:                                                                 # the foreground is 0 in front of the scaling layer, not -1
        fg = (mask == 1.0)[torch.arange(2 * b) % mask.shape[0]]
        for c in range(3):
            assert torch.equal(got[..., c][fg], torch.full_like(got[..., c][fg], (0.0 - lr.SHIFT[c]) / lr.SCALE[c]))


# ---------------------------------------------------------------------------------------------------------------- convolution
LAYERS = {"conv1": (4, 64, 11, 4, 2), "conv2": (64, 192, 5, 1, 2), "conv3": (192, 384, 3, 1, 1), "conv4": (384, 256, 3, 1, 1), "conv5": (256, 256, 3, 1, 1)}
CONV_CASES = [("conv1", 31, 31), ("conv1", 35, 38), ("conv1", 35, 39), ("conv2", 3, 3), ("conv2", 7, 7)] + [(l, s, s) for l in ("conv3", "conv4", "conv5")
                                                                                                           for s in (1, 3)]


@functools.lru_cache(maxsize=8)
def _conv_operands(layer, h, w, n, family, dtype):
    """(x NCHW, weight OIHW, bias) on the CPU, x and the weight already rounded to `dtype` (as float32), and the float64 reference before the ReLU
    with its bound"""
    cin, cout, k, stride, pad = LAYERS[layer]
    kt = cin * k * k
    if family == "exact":
        x, wt, bias = hash_ternary((n, cin, h, w), 11, 2.0 / 3.0), hash_ternary((cout, cin, k, k), 12, exact_w_density(kt)), hash_int((cout,), 13, 8)
    else:
        g = torch.Generator().manual_seed(h * 100 + w + n + kt)
        x, wt, bias = torch.randn(n, cin, h, w, generator=g), torch.randn(cout, cin, k, k, generator=g) * kt ** -0.5, torch.randn(cout, generator=g) + 0.5
    x, wt = x.to(dtype).float(), wt.to(dtype).float()
    ref = lr.conv2d(x.double(), wt.double(), bias.double(), stride, pad)
    mag = lr.conv2d(x.double().abs(), wt.double().abs(), bias.double().abs(), stride, pad)
    e = gamma_l(kt + 1 + 4) * mag
    return x, wt, bias, ref, e


@pytest.mark.parametrize("dtype", DTYPES3, ids=name_of)
@pytest.mark.parametrize("family", ["exact", "random"])
@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "linear"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_conv2d_relu(case, n, relu, family, dtype):
    _capi, lib = _lib()
    layer, h, w = case
    cin, cout, k, stride, pad = LAYERS[layer]
    x, wt, bias, ref, e = _conv_operands(layer, h, w, n, family, dtype)
    ho, wo = lr.out_size(h, k, stride, pad), lr.out_size(w, k, stride, pad)
    assert ref.shape == (n, cout, ho, wo)               # M = n ho wo is 1 .. 216: 128 once (35 x 38, n = 2), no tile multiple otherwise
    xd = x.permute(0, 2, 3, 1).contiguous().to(device="cuda", dtype=dtype)
    src, packed, bd = wt.contiguous().cuda(), torch.empty(cout, k * k, cin, dtype=dtype, device="cuda"), bias.cuda()
    _capi.check(lib.etainv_op_pack_weight(_capi.ptr(src), _capi.ptr(packed), cout, cin * k * k, 1, k * k, 1.0, None, _capi.dtype_code(dtype), _capi.stream_ptr()))
    assert torch.equal(packed.float().cpu(), wt.permute(0, 2, 3, 1).reshape(cout, k * k, cin))
    out = torch.full((n, ho, wo, cout), float("nan"), dtype=dtype, device="cuda")
    _capi.check(lib.etainv_op_conv2d_relu(_capi.ptr(xd), _capi.ptr(packed), _capi.ptr(bd), _capi.ptr(out), n, h, w, cin, cout, k, k, stride, pad, relu,
                                          _capi.dtype_code(dtype), _capi.stream_ptr()))
    got = out.cpu().permute(0, 3, 1, 2)
    want = ref.clamp(min=0) if relu else ref
    if family == "exact":
        assert float(ref.abs().max()) <= 256 and float(ref.abs().max()) >= 4
        assert torch.equal(got.double(), want), (got.double() - want).abs().max()
        return
    bound = U_RND[dtype] * (want.abs() + e) + e + ABS_FLOOR[dtype]
    r = worst(got, want, bound)
    print(f"lpips-conv {layer} {h}x{w} n={n} relu={relu} {name_of(dtype)}: worst |got - ref| / bound {r:.3f}")
    assert r <= 1.0


def test_conv2d_refusals_leave_the_output_alone():
    _capi, lib = _lib()
    x, wt, bias = torch.zeros(2, 7, 7, 64, dtype=torch.float16, device="cuda"), torch.zeros(192, 25, 64, dtype=torch.float16, device="cuda"), torch.zeros(192, device="cuda")
    out = torch.full((2, 7, 7, 192), 3.0, dtype=torch.float16, device="cuda")
    call = lambda **k: lib.etainv_op_conv2d_relu(*[{**dict(x=_capi.ptr(x), w=_capi.ptr(wt), b=_capi.ptr(bias), o=_capi.ptr(out), n=2, h=7, wd=7, cin=64, cout=192,
                                                           kh=5, kw=5, s=1, p=2, r=1, dt=_capi.F16, st=_capi.stream_ptr()), **k}[a]
                                                   for a in ("x", "w", "b", "o", "n", "h", "wd", "cin", "cout", "kh", "kw", "s", "p", "r", "dt", "st")])
    err = lambda: lib.etainv_last_error().decode()
    assert call(cin=48) != 0 and "multiple of 32" in err()
    assert call(cout=190) != 0 and "multiple of 4" in err()
    assert call(h=2, p=0) != 0 and "smaller than 1 x 1" in err()
    assert call(x=_capi.ptr(x) + 2) != 0 and "16-byte aligned" in err()
    assert call(w=None) != 0 and "null pointer" in err()
    assert call(s=2) != 0 and "stride" in err()
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())


# ---------------------------------------------------------------------------------------------------------------- max pooling
@pytest.mark.parametrize("dtype", DTYPES3, ids=name_of)
@pytest.mark.parametrize("shape", [(15, 15, 64), (16, 16, 64), (7, 7, 192), (3, 3, 192), (16, 7, 64), (5, 9, 384)], ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_maxpool3s2(shape, dtype):
    _capi, lib = _lib()
    h, w, c = shape
    g = torch.Generator().manual_seed(h * 100 + w)
    x = (torch.randn(3, h, w, c, generator=g) * 0.5 - 3).to(dtype)                # negative: a maximum that starts from 0 fails
    x[0, :3, :3, :8] = -5.0                                                       # a window of equal values
    want = F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1).contiguous().to(dtype)
    ho, wo = lr.pool_size(h), lr.pool_size(w)
    assert want.shape == (3, ho, wo, c) and float((want < 0).float().mean()) > 0.9
    out = torch.full((3, ho, wo, c), float("nan"), dtype=dtype, device="cuda")
    xd = x.cuda()
    _capi.check(lib.etainv_op_maxpool3s2(_capi.ptr(xd), _capi.ptr(out), 3, h, w, c, _capi.dtype_code(dtype), _capi.stream_ptr()))
    assert torch.equal(out.cpu().view(INT[dtype]), want.view(INT[dtype]))


# ---------------------------------------------------------------------------------------------------------------- distance
def _features(b, pixels, c, dtype, seed):
    """[2 b][pixels][c] post-ReLU-like features (half the entries zero): rows b .. 2b-1 = rows 0 .. b-1 plus noise, clamped; and lin weights U(0, 4 / c)"""
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(b, pixels, c, generator=g).clamp(min=0) * 3
    edit = (src + 0.3 * torch.randn(b, pixels, c, generator=g)).clamp(min=0)
    return torch.cat([src, edit]).to(dtype), torch.rand(c, generator=g) * (4.0 / c)


def _dist64(f, w):
    b = f.shape[0] // 2
    return lr.tap_distance(f[:b].double().transpose(1, 2)[..., None], f[b:].double().transpose(1, 2)[..., None], w)


def _bits(t):
    return t.cpu().view(torch.int64)


@pytest.mark.parametrize("dtype", DTYPES3, ids=name_of)
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("pixels", [1, 9, 49, 225])
@pytest.mark.parametrize("c", [64, 192, 384, 256])
def test_layer_distance(c, pixels, b, dtype):
    from metrics.lpips import layer_distance
    f, w = _features(b, pixels, c, dtype, seed=c * 1000 + pixels * 10 + b)
    if pixels > 1:
        f[0, 0] = 0                                                               # an all-zero pixel on the source side of pair 0: the epsilon path
    fd, wd = f.cuda(), w.cuda()
    got = layer_distance(fd, wd)
    want = _dist64(f, w)
    assert got.dtype == torch.float64 and got.shape == (b,) and bool(torch.isfinite(got).all()) and float(want.min()) > 0
    err, bound = float((got.cpu() - want).abs().max()), 1e-12 * 4 * float(w.max())
    print(f"lpips-distance c={c} pixels={pixels} b={b} {name_of(dtype)}: max |s - s_64| {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert torch.equal(_bits(layer_distance(fd, wd)), _bits(got))                                           # run to run
    assert torch.equal(_bits(layer_distance(torch.cat([fd[b:], fd[:b]]), wd)), _bits(got))                  # the sides swapped
    same = layer_distance(torch.cat([fd[b:], fd[b:]]), wd)
    assert bool((same == 0.0).all()) and not bool(torch.signbit(same).any())                                # exactly 0.0 for identical features
    for i in range(b):                                                                                      # row by row against single-pair calls
        assert torch.equal(_bits(layer_distance(torch.stack([fd[i], fd[b + i]]), wd)), _bits(got[i:i + 1])), i
    f2, w2 = _features(b, 9, 64, dtype, seed=5)                                                             # a second tap added into the first's result
    second = layer_distance(f2.cuda(), w2.cuda())
    both = layer_distance(f2.cuda(), w2.cuda(), out=got.clone())
    assert torch.equal(_bits(both), _bits(got + second))


def test_layer_distance_epsilon_is_added_to_the_norm():
    from metrics.lpips import layer_distance
    f = torch.zeros(2, 2, 64)
    f[1, 0, :4] = torch.tensor([3.0, 0.0, 4.0, 0.0])              # pixel 0: zero against (3, 0, 4, 0, 0 ...); pixel 1: zero against zero
    w = torch.zeros(64)
    w[:4] = torch.tensor([0.5, 0.25, 1.0, 2.0])
    for dtype in DTYPES3:
        got = float(layer_distance(f.to(dtype).cuda(), w.cuda())[0])
        assert got == pytest.approx((0.5 * 0.36 + 1.0 * 0.64) / 2, rel=1e-10)
    tiny = torch.zeros(2, 1, 64)
    tiny[0, 0, :4] = 1e-10                                        # |f| = 2e-10: f / (|f| + 1e-10) = 1/3 per channel, a clamp would give 1/2
    got = float(layer_distance(tiny.cuda(), torch.ones(64).cuda())[0])
    assert got == pytest.approx(4 / 9, rel=1e-6)                  # (1e-10 as fp32 is not exactly 1e-10)
