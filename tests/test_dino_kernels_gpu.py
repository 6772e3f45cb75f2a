"""The kernels of csrc/dino.hip, each against tests/dino_ref.py in float64 (pinned on the CPU by tests/test_dino_ref.py).  u = 2^-24 throughout.

preprocess  Per element of the fp32 rows, counted: the range map (x - lo) / (hi - lo) is a subtraction and a division, 2 u on a value in [0, 1];
            each pass rounds its weights to fp32 (they are non-negative and sum to 1: at most u on the weighted mean of values in [0, 1]) and does
            one FMA per tap (at most u each, the partial sums staying in [0, 1]), taps + 1 per pass; so the resized value carries at most
            2 + 2 (taps + 1) = 2 (taps + 2) units of u.  (v - mean) / std runs in float64 and is rounded once: the error above divided by std_c,
            plus one rounding of a result below 1 / std_c in magnitude -- the bound allows two:  (2 (taps + 2) + 2) u / std_c.
            A 16-bit row gets that bound plus half an ulp of the float64 value in that type.
gelu_erf    |y - x Phi(x)| <= 1.8e-7 |x| / 2 (the erf error stated in common.h, times the factor x / 2 it is multiplied by) + 2 u |x| (the
            product h s and the sum h s + h, one rounding each, each at most |x| in magnitude) + half an ulp of y in a 16-bit output.
selfsim     Against dino_ref.score on the same stored keys.  Per entry: |dot_gpu - dot_64| <= d u sum_k |a_k b_k| (any order of d fp32
            additions: the counted rule of tests/gemm_ref.py); a squared norm is a sum of d non-negative terms, relative error d u, its root
            (d / 2 + 1) u, the product of two norms (d + 3) u, the division one more: eps_ij = d u A_ij / N_ij + |cos_ij| (d + 4) u, times
            1 + 2 (d + 4) u for the second order.  Both matrices: eps = eps_src + eps_edit on the difference Delta, and the score moves by at
            most mean(2 |Delta| eps + eps^2); the float64 sums add 1e-14 relative.  The test computes this bound from its inputs.
            exact family: every key row is +- 2^k e_m, so dots, norms and cosines are exactly 0 or +-1, every squared difference is 0, 1 or 4,
            and the score equals float64(count) / n^2 bit for bit: indexing, the i, j >= n masks and the doubling of off-diagonal tiles."""
import functools
import math

import pytest
import torch

from tests import dino_ref as dr

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
name_of = lambda dt: str(dt).split(".")[-1]


def half_ulp(v, dtype):
    """half an ulp of |v| (float64 tensor) in a 16-bit type; 0 for float32 (whose rounding the bounds count in u)"""
    if dtype == torch.float32:
        return torch.zeros_like(v)
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** emin)))
    return torch.pow(2.0, e - mant - 1)


# ---------------------------------------------------------------------------------------------------------------- preprocess
@functools.lru_cache(maxsize=None)
def _images(b, s, lo, hi):
    x = dr.make_images(b, s, lo, hi, seed=7 * s + b)[0]
    assert x.min() >= lo and x.max() <= hi
    return x


@functools.lru_cache(maxsize=None)
def _ref_rows(b, s, r, p, lo, hi, antialias):
    return dr.patch_rows(dr.preprocess(_images(b, s, lo, hi), lo, hi, r, antialias), p)


RESIZES = [(20, 32, 8), (64, 224, 8), (224, 224, 8), (300, 224, 8), (512, 224, 8)]
PRE_CASES = [(s, r, p, b, aa, rng) for s, r, p in RESIZES for b in (1, 3) for aa in (True, False) for rng in ((-1, 1), (0, 255))]
PRE_CASES += [(512, 224, 16, 1, aa, (-1, 1)) for aa in (True, False)]                 # patch 16: rows of 768


@pytest.mark.parametrize("s,r,p,b,antialias,rng", PRE_CASES)
def test_preprocess_rows(s, r, p, b, antialias, rng):
    from metrics.dino_vit_structure import dino_preprocess, resize_tables
    x = _images(b, s, *rng).cuda()
    ref = _ref_rows(b, s, r, p, rng[0], rng[1], antialias)
    taps = resize_tables(s, r, antialias)[1].shape[1]
    std = torch.tensor(dr.STD, dtype=torch.float64).repeat_interleave(p * p)
    base = (2 * (taps + 2) + 2) * U / std
    for dtype in DTYPES:
        rows = dino_preprocess(x, rng, r, p, dtype, antialias).cpu()
        assert rows.shape == ref.shape == (b * (r // p) ** 2, 3 * p * p) and rows.dtype == dtype
        err = (rows.double() - ref).abs()
        worst = (err / (base + half_ulp(ref, dtype))).max().item()
        print(f"dino-preprocess {s}->{r} p={p} B={b} antialias={antialias} range={rng} {name_of(dtype)}: {taps} taps, worst error / bound {worst:.3f}")
        assert worst <= 1.0


def test_preprocess_clamps_a_table_with_out_of_range_entries():
    from etainv import _capi
    from metrics.dino_vit_structure import _band_rows, resize_tables
    lib = _capi.load()
    s, r, p, b = 64, 224, 8, 2
    bounds, coef = resize_tables(s, r, True)
    g = torch.Generator().manual_seed(0)
    bad = torch.stack([torch.randint(-1000, 100000, (r,), generator=g), torch.randint(-5, 1000, (r,), generator=g)], 1).to(torch.int32).cuda()
    w = torch.randn(r, coef.shape[1], generator=g).cuda()
    x = _images(b, s, -1, 1).cuda()
    rows = torch.zeros(b * (r // p) ** 2, 3 * p * p, dtype=torch.float16, device="cuda")
    _capi.check(lib.etainv_dino_preprocess(_capi.ptr(x), b, s, r, p, -1.0, 1.0, _capi.ptr(bad), _capi.ptr(w), coef.shape[1], _capi.ptr(bad),
                                           _capi.ptr(w), coef.shape[1], _band_rows(bounds, p), _capi.ptr(rows), _capi.F16, _capi.stream_ptr()))
    torch.cuda.synchronize()
    assert rows.cpu().shape == (b * 784, 192)


# ---------------------------------------------------------------------------------------------------------------- erf GELU
@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
@pytest.mark.parametrize("n", [1, 255, 4097])
def test_gelu_erf(n, dtype):
    from etainv import _capi
    lib = _capi.load()
    x = (torch.linspace(-6, 6, n, dtype=torch.float64) if n > 1 else torch.tensor([1.3], dtype=torch.float64)).to(dtype)
    x64 = x.double()
    ref = 0.5 * x64 * (1.0 + torch.erf(x64 / math.sqrt(2.0)))
    bound = 1.8e-7 * x64.abs() / 2 + 2 * U * x64.abs() + half_ulp(ref, dtype)
    for inplace in (False, True):
        src = x.cuda()
        dst = src if inplace else torch.full_like(src, 7.0)
        _capi.check(lib.etainv_op_gelu_erf(_capi.ptr(src), _capi.ptr(dst), n, _capi.dtype_code(dtype), _capi.stream_ptr()))
        err = (dst.cpu().double() - ref).abs()
        worst = (err / bound.clamp(min=1e-300)).max().item()
        print(f"gelu_erf n {n} inplace {inplace} {name_of(dtype)}: worst error / bound {worst:.3f}")
        assert (err <= bound).all()


# ---------------------------------------------------------------------------------------------------------------- self-similarity
def _launch(keys, eps=dr.EPS, d=None, norms=False):
    from metrics.dino_vit_structure import key_self_similarity_mse
    out = key_self_similarity_mse(keys, eps, d, return_norms=norms)
    return (out[0].cpu(), out[1].cpu()) if norms else out.cpu()


def _score_and_bound(keys, d):
    """(float64 scores [B], bound [B], float64 norms [2 B][n]) from the stored keys: see the module docstring"""
    k = keys.double()
    b = k.shape[0] // 2
    norm = k.norm(dim=-1, keepdim=True)
    prod = (norm @ norm.transpose(-1, -2)).clamp(min=dr.EPS)
    cos = (k @ k.transpose(-1, -2)) / prod
    a = k.abs() @ k.abs().transpose(-1, -2)
    eps = (d * U * a / prod + cos.abs() * (d + 4) * U) * (1 + 2 * (d + 4) * U)
    delta, e = cos[b:] - cos[:b], eps[b:] + eps[:b]
    score = delta.square().mean((-1, -2))
    return score, (2 * delta.abs() * e + e * e).mean((-1, -2)) + 1e-14 * score, norm[..., 0]


@pytest.mark.parametrize("d", [64, 128, 768])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 129, 785])
def test_selfsim_random(n, d):
    for dtype in DTYPES:
        for b in (1, 3):
            keys = dr.random_keys(b, n, d, dtype, seed=1000 * n + d + b)
            ref, bound, norm64 = _score_and_bound(keys, d)
            assert (ref - dr.score(keys[:b], keys[b:])).abs().max() <= 1e-13
            got, norms = _launch(keys.cuda(), norms=True)
            assert got.dtype == torch.float64 and got.shape == (b,) and norms.shape == (2 * b, n) and norms.dtype == torch.float32
            worst = ((got - ref).abs() / bound.clamp(min=1e-300)).max().item()
            print(f"dino-selfsim random n={n} d={d} B={b} {name_of(dtype)}: score {ref[0]:.4e}, worst |diff| / bound {worst:.3f} (bound {bound[0]:.2e})")
            assert n == 1 or ref.min() > 0
            assert ((got - ref).abs() <= bound).all()
            assert ((norms.double() - norm64).abs() <= (d / 2 + 2) * U * norm64).all()
            # the keys as the middle third of a [2 B][n][3 d] qkv tensor (ld = 3 d, column offset d): bit for bit the contiguous result
            qkv = torch.full((2 * b, n, 3 * d), float("nan"), dtype=dtype, device="cuda")
            qkv[:, :, d:2 * d] = keys.cuda()
            view = qkv[:, :, d:2 * d]
            assert not view.is_contiguous() and view.stride() == (3 * d * n, 3 * d, 1)
            assert torch.equal(_launch(view).view(torch.int64), got.view(torch.int64))


def _exact_keys(b, n, d, dtype, seed):
    """(keys [2 b][n][d] with rows +- 2^k e_m, the exact count of the squared differences per pair)"""
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(0, min(d, 6), (2 * b, n), generator=g)              # few directions: many pairs share one
    sign = torch.randint(0, 2, (2 * b, n), generator=g) * 2 - 1
    mag = torch.pow(2.0, torch.randint(-3, 4, (2 * b, n), generator=g).double())
    keys = torch.zeros(2 * b, n, d, dtype=torch.float64)
    keys.scatter_(2, m[..., None], (sign * mag)[..., None])
    cos = (m[:, :, None] == m[:, None, :]).long() * sign[:, :, None] * sign[:, None, :]
    count = (cos[b:] - cos[:b]).square().sum((-1, -2))
    return keys.to(dtype), count


@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
@pytest.mark.parametrize("n", [17, 65, 785])
def test_selfsim_exact(n, dtype):
    for b, d in ((1, 64), (3, 128)):
        keys, count = _exact_keys(b, n, d, dtype, seed=n + b)
        assert set((dr.self_sim(keys) * 1.0).unique().tolist()) <= {-1.0, 0.0, 1.0} and count.min() > 0
        want = torch.tensor([float(c) / n ** 2 for c in count.tolist()], dtype=torch.float64)
        got, norms = _launch(keys.cuda(), norms=True)
        assert torch.equal(got.view(torch.int64), want.view(torch.int64)), (n, b, d, got.tolist(), want.tolist())
        assert torch.equal(norms.double(), keys.double().norm(dim=-1))


@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
def test_selfsim_zero_row_in_the_source(dtype):
    from etainv import _capi
    n, d = 65, 128
    keys = dr.random_keys(1, n, d, dtype, seed=5)
    keys[0, 40] = 0
    ref, bound, _ = _score_and_bound(keys, d)
    got = _launch(keys.cuda())
    assert torch.isfinite(got).all() and ((got - ref).abs() <= bound).all()
    with pytest.raises(_capi.EtainvError, match="eps must be positive"):
        _launch(keys.cuda(), eps=0.0)


def test_selfsim_repeats_and_does_not_depend_on_the_batch():
    for dtype in DTYPES:
        n, d, b = 129, 128, 3
        keys = dr.random_keys(b, n, d, dtype, seed=11).cuda()
        full, again = _launch(keys), _launch(keys)
        assert torch.equal(full.view(torch.int64), again.view(torch.int64))
        for i in range(b):
            alone = _launch(torch.stack([keys[i], keys[b + i]]))
            assert torch.equal(alone.view(torch.int64), full[i:i + 1].view(torch.int64)), (name_of(dtype), i)
