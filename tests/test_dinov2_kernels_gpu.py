"""The two kernels dinovitstruct_v2 adds, each against float64.  u = 2^-24 throughout.

preprocess  etainv_dinov2_preprocess against tests/dinov2_ref.py (dino_ref's resize and normalisation, patch rows of 14 x 14) under the counted
            bound tests/test_dino_kernels_gpu.py uses for the p = 8 kernel, restated: the range map (x - lo) / (hi - lo) is a subtraction and a
            division, 2 u on a value in [0, 1]; each pass rounds its weights to fp32 (non-negative, summing to 1: at most u on the weighted mean)
            and does one FMA per tap (at most u each), taps + 1 per pass; so the resized value carries at most 2 + 2 (taps + 1) = 2 (taps + 2)
            units of u.  (v - mean) / std runs in float64 and is rounded once: the error above divided by std_c plus one rounding of a result
            below 1 / std_c in magnitude -- the bound allows two: (2 (taps + 2) + 2) u / std_c, plus half an ulp of the float64 value in a
            16-bit type.  The output buffer, one guard row included, is pre-filled with NaN: columns 0 .. 587 must hold the values, columns
            588 .. 639 exactly zero, the guard row nothing.
fused       etainv_op_layerscale_add_layernorm.  x_out: one fp32 FMA and one rounding to T put it within u |v| + half an ulp of T of the float64
            value v = x + g y: the test allows one ulp of T (fp32: one ulp of fp32).  The `exact` family (small integers, gamma a power of two:
            every value representable in bf16) must match bit for bit.  h_out against norm_ref.ln_bound evaluated on the STORED x_out (the bound
            of tests/test_norm_gpu.py for the two-pass row LayerNorm: 24 terms per lane and 6 butterfly steps, which is this kernel's chain in
            all three types); in fp16 and bf16 it must equal etainv_op_layernorm(x_out) bit for bit.  x_out = null and x_out == x (in place)
            give the same h_out, and two runs the same bits."""
import functools

import pytest
import torch

from tests import dinov2_ref as v2
from tests import norm_ref as nr

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
name_of = lambda dt: str(dt).split(".")[-1]
MANT = {torch.float16: (10, -14), torch.bfloat16: (7, -126), torch.float32: (23, -126)}
KP = 640


def ulp(v, dtype):
    """one ulp of |v| (float64 tensor) in `dtype` (a subnormal step below the smallest normal)"""
    mant, emin = MANT[dtype]
    return torch.pow(2.0, torch.floor(torch.log2(v.abs().clamp(min=2.0 ** emin))) - mant)


# ---------------------------------------------------------------------------------------------------------------- preprocess
@functools.lru_cache(maxsize=None)
def _images(b, s, lo, hi):
    x = v2.make_images(b, s, lo, hi, seed=7 * s + b)[0]
    assert x.min() >= lo and x.max() <= hi
    return x


@functools.lru_cache(maxsize=None)
def _ref_rows(b, s, r, lo, hi, antialias):
    return v2.patch_rows(v2.preprocess(_images(b, s, lo, hi), lo, hi, r, antialias), 14)


PRE_CASES = [(s, r, 2, aa, (-1, 1)) for r in (28, 42, 224) for s in (20, 64, r, 256) for aa in (True, False)] + [(64, 42, 3, True, (0, 255))]


@pytest.mark.parametrize("s,r,b,antialias,rng", PRE_CASES)
def test_preprocess_rows(s, r, b, antialias, rng):
    from etainv import _capi
    from metrics.dino_vit_structure import _device_tables, dinov2_preprocess, resize_tables
    lib = _capi.load()
    x = _images(b, s, *rng).cuda()
    ref = _ref_rows(b, s, r, rng[0], rng[1], antialias)
    taps = resize_tables(s, r, antialias)[1].shape[1]
    assert taps == 1 if s == r else taps >= 2
    std = torch.tensor(v2.dr.STD, dtype=torch.float64).repeat_interleave(196)
    base = (2 * (taps + 2) + 2) * U / std
    n = b * (r // 14) ** 2
    tb, tc, ksize, band = _device_tables(s, r, 14, antialias, str(x.device))
    for dtype in DTYPES:
        buf = torch.full((n + 1, KP), float("nan"), dtype=dtype, device="cuda")
        _capi.check(lib.etainv_dinov2_preprocess(_capi.ptr(x), b, s, r, float(rng[0]), float(rng[1]), _capi.ptr(tb), _capi.ptr(tc), ksize, _capi.ptr(tb),
                                                 _capi.ptr(tc), ksize, band, _capi.ptr(buf), _capi.dtype_code(dtype), _capi.stream_ptr()))
        rows = buf.cpu()
        assert torch.isnan(rows[n]).all()                                                 # nothing behind the last row
        assert not torch.isnan(rows[:n]).any() and (rows[:n, 588:] == 0).all()
        err = (rows[:n, :588].double() - ref).abs()
        worst = (err / (base + ulp(ref, dtype) / 2 * (dtype != torch.float32))).max().item()
        print(f"dinov2-preprocess {s}->{r} B={b} antialias={antialias} range={rng} {name_of(dtype)}: {taps} taps, {band} band rows, worst error / bound {worst:.3f}")
        assert worst <= 1.0
        assert torch.equal(dinov2_preprocess(x, rng, r, dtype, antialias).cpu(), rows[:n])  # the library's call is this launch


def test_preprocess_clamps_a_table_with_out_of_range_entries():
    from etainv import _capi
    from metrics.dino_vit_structure import _band_rows, resize_tables
    lib = _capi.load()
    s, r, b = 64, 224, 2
    bounds, coef = resize_tables(s, r, True)
    g = torch.Generator().manual_seed(0)
    bad = torch.stack([torch.randint(-1000, 100000, (r,), generator=g), torch.randint(-5, 1000, (r,), generator=g)], 1).to(torch.int32).cuda()
    w = torch.randn(r, coef.shape[1], generator=g).cuda()
    x = _images(b, s, -1, 1).cuda()
    rows = torch.full((b * 256 + 1, KP), float("nan"), dtype=torch.float16, device="cuda")
    _capi.check(lib.etainv_dinov2_preprocess(_capi.ptr(x), b, s, r, -1.0, 1.0, _capi.ptr(bad), _capi.ptr(w), coef.shape[1], _capi.ptr(bad), _capi.ptr(w),
                                             coef.shape[1], _band_rows(bounds, 14), _capi.ptr(rows), _capi.F16, _capi.stream_ptr()))
    torch.cuda.synchronize()
    out = rows.cpu()
    assert torch.isnan(out[-1]).all() and (out[:-1, 588:] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- the fused kernel
EPS = 1e-6
FAMILIES = ["loguniform", "tiny", "mixed"]


def _gammas(c, family, seed):
    g = torch.Generator().manual_seed(seed)
    if family == "tiny":
        return torch.full((c,), 1e-5)
    mag = torch.pow(10.0, -5.0 * torch.rand(c, generator=g))
    return mag if family == "loguniform" else mag * (torch.randint(0, 2, (c,), generator=g).float() * 2 - 1)


def _fused(y, ls, x, gamma, beta, mode):
    """mode "out": x_out a buffer of its own; "null": no x_out; "inplace": x_out == x (on a copy of x).  Outputs are pre-filled with NaN and carry
    a guard row.  -> (x_out or None, h_out), guard rows checked and cut"""
    from etainv import _capi
    lib = _capi.load()
    rows, c = x.shape
    h = torch.full((rows + 1, c), float("nan"), dtype=x.dtype, device=x.device)
    if mode == "inplace":
        xo = torch.cat([x, torch.full((1, c), float("nan"), dtype=x.dtype, device=x.device)])
        src = xo
    else:
        xo = torch.full((rows + 1, c), float("nan"), dtype=x.dtype, device=x.device) if mode == "out" else None
        src = x
    _capi.check(lib.etainv_op_layerscale_add_layernorm(_capi.ptr(y), _capi.ptr(ls), _capi.ptr(src), _capi.ptr(gamma), _capi.ptr(beta), EPS, _capi.ptr(xo),
                                                       _capi.ptr(h), rows, c, _capi.dtype_code(x.dtype), _capi.stream_ptr()))
    assert torch.isnan(h[rows]).all() and not torch.isnan(h[:rows]).any()
    if xo is not None:
        assert torch.isnan(xo[rows]).all() and not torch.isnan(xo[:rows]).any()
    return (None if xo is None else xo[:rows]), h[:rows]


def _layernorm(x, gamma, beta):
    from etainv import _capi
    lib = _capi.load()
    out = torch.empty_like(x)
    _capi.check(lib.etainv_op_layernorm(_capi.ptr(x), _capi.ptr(gamma), _capi.ptr(beta), _capi.ptr(out), x.shape[0], x.shape[1], EPS,
                                        _capi.dtype_code(x.dtype), _capi.stream_ptr()))
    return out


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("rows", [1, 3, 5, 514])
@pytest.mark.parametrize("c", [64, 128, 384, 768, 1024, 1536])
def test_layerscale_add_layernorm(c, rows):
    gamma, beta = (t.cuda() for t in nr.ln_params(c))
    for dtype in DTYPES:
        x = nr.row_input(rows, c, dtype, "random", seed=rows + c).cuda()
        y = nr.row_input(rows, c, dtype, "random", seed=rows + c + 1).cuda()
        for family in FAMILIES:
            ls = _gammas(c, family, seed=c + rows).cuda()
            xo, h = _fused(y, ls, x, gamma, beta, "out")
            v = x.double() + ls.double() * y.double()
            worst_x = ((xo.double() - v).abs() / ulp(v, dtype)).max().item()
            ref, bound, _ = nr.ln_bound(xo, gamma, beta, EPS, dtype)
            worst_h = nr.worst(h, ref, bound)
            print(f"layerscale+ln c={c} rows={rows} {family} {name_of(dtype)}: x_out worst error / ulp {worst_x:.3f}, h_out worst error / bound {worst_h:.3f}")
            assert worst_x <= 1.0
            assert worst_h <= 1.0
            if dtype != torch.float32:
                assert _same_bits(h, _layernorm(xo, gamma, beta))
            _, h_null = _fused(y, ls, x, gamma, beta, "null")
            x_in, h_in = _fused(y, ls, x, gamma, beta, "inplace")
            assert _same_bits(h_null, h) and _same_bits(h_in, h) and _same_bits(x_in, xo)
            xo2, h2 = _fused(y, ls, x, gamma, beta, "out")
            assert _same_bits(xo2, xo) and _same_bits(h2, h)


@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
def test_layerscale_add_exact(dtype):
    """x and y integers in [-8, 8], gamma +- 2^-k with k <= 3: x + g y is a multiple of 1/8 below 9.1 in magnitude, exact in bf16"""
    for c, rows in ((64, 5), (768, 514), (1536, 3)):
        g = torch.Generator().manual_seed(c)
        x = torch.randint(-8, 9, (rows, c), generator=g).to(dtype).cuda()
        y = torch.randint(-8, 9, (rows, c), generator=g).to(dtype).cuda()
        ls = (torch.pow(2.0, -torch.randint(0, 4, (c,), generator=g).float()) * (torch.randint(0, 2, (c,), generator=g).float() * 2 - 1)).cuda()
        gamma, beta = (t.cuda() for t in nr.ln_params(c))
        xo, h = _fused(y, ls, x, gamma, beta, "out")
        want = x.double() + ls.double() * y.double()
        assert torch.equal(want.to(dtype).double(), want)
        assert _same_bits(xo, want.to(dtype))
        ref, bound, _ = nr.ln_bound(xo, gamma, beta, EPS, dtype)
        assert nr.worst(h, ref, bound) <= 1.0
