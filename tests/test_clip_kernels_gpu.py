"""The four kernels of csrc/clip.hip, each against tests/clip_ref.py (pinned on the CPU by tests/test_clip_ref.py).

preprocess  the resized bytes equal the integer restatement of Pillow's bicubic resize bit for bit; patch rows: an fp32 row is within 2 fp32 ulp of
            the float64 formula, a 16-bit row equals the rounded float64 value except where that value lies within 2 fp32 ulp of a rounding boundary
            (either neighbour is accepted there; such elements are counted and capped at 1 % -- the count depends on the inputs only).
attention   random inputs against float64 with the error measure and tolerances of tests/attention_ref.py; a peaked family (one key per query
            30 above the rest in the logit: the output is that V row to one rounding); an exact family (all keys equal, all V rows one
            small-integer vector: the output is that vector bit for bit, which a padded key slot entering the sum would break).  qkv and out are
            views into larger allocations whose surroundings hold NaN / a sentinel.
head        against float64 within 8 eps32 sqrt(d) on the unit vector (L2 and per element); a row's result is bit-identical at B = 1 and B = 5.
scores      within 1e-6 of float64; acc exact, an exact tie is 0.0; bit-identical across runs, across B and between a mode's own launch and the
            all-four launch."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import attention_ref as ar
from tests import clip_ref as cr

pytestmark = pytest.mark.gpu
EPS32 = 2.0 ** -23
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
RESIZES = [(512, 224), (96, 224), (64, 32), (48, 32), (37, 32), (32, 32)]
PAD = 64            # elements around every view: 16-byte aligned in all three types


# ---------------------------------------------------------------------------------------------------------------- preprocess
@functools.lru_cache(maxsize=None)
def _images(b, s, lo, hi):
    x = cr.make_images(b, s, lo, hi, seed=s + b)
    assert (x < lo).any() and (x > hi).any()
    return x


@functools.lru_cache(maxsize=None)
def _ref_u8(b, s, r, lo, hi):
    return cr.preprocess_u8(_images(b, s, lo, hi), lo, hi, r)


@pytest.mark.parametrize("rng", [(-1, 1), (0, 1)])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("s,r", RESIZES)
def test_preprocess_bytes_equal_pillows_integer_resize(s, r, b, rng):
    from metrics.clip_similarity import clip_preprocess
    _, u8 = clip_preprocess(_images(b, s, *rng).cuda(), rng, r, 16, torch.float16, return_u8=True)
    ref = _ref_u8(b, s, r, *rng)
    got = u8.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.uint8
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} bytes differ"


def test_preprocess_truncates_where_rounding_would_go_up():
    from metrics.clip_similarity import clip_preprocess
    for lo, hi in ((-1, 1), (0, 1)):
        x = cr.truncation_images(32, lo, hi)
        _, u8 = clip_preprocess(x.cuda(), (lo, hi), 32, 16, torch.float16, return_u8=True)
        k = (torch.arange(3 * 32 * 32) % 255).reshape(1, 3, 32, 32).numpy().astype(np.uint8)
        assert np.array_equal(cr.to_u8(x, lo, hi), k)                 # the premise: k + 0.999 truncates to k
        assert np.array_equal(u8.cpu().numpy(), k)


def _rows_check(got, f64, dtype):
    """(violations, excepted elements): see the module docstring"""
    ulp = torch.from_numpy(np.spacing(np.abs(f64.numpy()).astype(np.float32)).astype(np.float64))
    if dtype == torch.float32:
        return int(((got.double() - f64).abs() > 2 * ulp).sum()), 0
    lo16, hi16 = (f64 - 2 * ulp).to(dtype), (f64 + 2 * ulp).to(dtype)
    firm = lo16 == hi16
    bad = (firm & (got != f64.to(dtype))) | (~firm & (got != lo16) & (got != hi16))
    return int(bad.sum()), int((~firm).sum())


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("s,r,p", [(48, 32, 16), (48, 32, 32), (37, 28, 14), (32, 32, 16)])
def test_preprocess_patch_rows(s, r, p, dtype):
    from metrics.clip_similarity import clip_preprocess
    b, rng = 3, (-1, 1)
    rows, u8 = clip_preprocess(_images(b, s, *rng).cuda(), rng, r, p, dtype, return_u8=True)
    ref_u8 = _ref_u8(b, s, r, *rng)
    assert np.array_equal(u8.cpu().numpy(), ref_u8)
    f64 = cr.patch_rows(ref_u8, p)
    kp, k3 = cr.k_padded(p), 3 * p * p
    rows = rows.cpu()
    assert rows.shape == f64.shape == (b * (r // p) ** 2, kp) and rows.dtype == dtype and kp % 64 == 0
    assert (rows[:, k3:] == 0).all() and (f64[:, k3:] == 0).all()
    bad, excepted = _rows_check(rows[:, :k3], f64[:, :k3], dtype)
    n = f64[:, :k3].numel()
    print(f"clip-preprocess rows {s}->{r} p={p} {dtype}: violations {bad}, excepted {excepted} of {n}")
    assert excepted <= 0.01 * n, "the inputs put more than 1 % of the elements on a rounding boundary"
    assert bad == 0


# ---------------------------------------------------------------------------------------------------------------- attention
def _launch_attention(qkv, heads):
    """qkv (b, n, 3 heads 64) on the CPU -> out (b, n, heads 64) on the CPU; both device tensors are views into larger allocations"""
    from etainv import _capi
    lib = _capi.load()
    b, n, c3 = qkv.shape
    dtype, sentinel = qkv.dtype, 12345.0
    big_in = torch.full((qkv.numel() + 2 * PAD,), float("nan"), dtype=dtype, device="cuda")
    big_in[PAD:PAD + qkv.numel()] = qkv.reshape(-1).cuda()
    big_out = torch.full((b * n * c3 // 3 + 2 * PAD,), sentinel, dtype=dtype, device="cuda")
    vin, vout = big_in[PAD:PAD + qkv.numel()], big_out[PAD:PAD + b * n * c3 // 3]
    _capi.check(lib.etainv_op_vit_attention(vin.data_ptr(), vout.data_ptr(), b, n, heads, 64, _capi.dtype_code(dtype), _capi.stream_ptr()))
    torch.cuda.synchronize()
    assert (big_out[:PAD] == sentinel).all() and (big_out[-PAD:] == sentinel).all(), "wrote outside out"
    out = vout.reshape(b, n, c3 // 3).cpu()
    assert torch.isfinite(out.float()).all(), "a row >= n or a padded key slot reached the output"
    return out


NS = [1, 5, 17, 50, 64, 65, 197, 257]
SHAPES = [(b, heads) for b in (1, 3) for heads in (1, 2)]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("n", NS)
def test_vit_attention_random(n, dtype):
    for b, heads in SHAPES:
        qkv = ar.random_qkv(b, n, heads, 64, dtype, seed=1000 * n + 10 * b + heads)
        out = _launch_attention(qkv, heads)
        ref = ar.ref_self_attention(qkv, heads, dt=torch.float64)
        ar.check_attention(out, ref, heads, 64, dtype, label=f"vit n={n} b={b} heads={heads}")


def _peaked(b, n, heads, dtype, seed):
    """(qkv, peak key of every (row, query, head)): keys c u_j on random directions u_j, query i = c u_j(i)"""
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(b, n, heads, 64, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    peak = (7 * torch.arange(n) + 3) % n
    c = 40.0
    q, k, v = c * u[:, peak], c * u, torch.randn(b, n, heads, 64, generator=g)
    return torch.cat([t.reshape(b, n, -1) for t in (q, k, v)], -1).to(dtype), peak


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("n", NS)
def test_vit_attention_peaked(n, dtype):
    for b, heads in SHAPES:
        qkv, peak = _peaked(b, n, heads, dtype, seed=n + b + heads)
        c = heads * 64
        q, k, v = (t.double().reshape(b, n, heads, 64) for t in qkv.split(c, -1))
        s = torch.einsum("bihd,bjhd->bhij", q, k) / 8
        top = s.gather(-1, peak.view(1, 1, n, 1).expand(b, heads, n, 1)).squeeze(-1)
        rest = s.scatter(-1, peak.view(1, 1, n, 1).expand(b, heads, n, 1), float("-inf")).amax(-1)
        assert n == 1 or (top - rest).min() >= 30, "premise: the peak key leads by 30 in the logit"
        out = _launch_attention(qkv, heads)
        want = v[:, peak].reshape(b, n, c)
        torch.testing.assert_close(out.double(), want, rtol=float(torch.finfo(dtype).eps), atol=0)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("n", NS)
def test_vit_attention_exact(n, dtype):
    for b, heads in SHAPES:
        g = torch.Generator().manual_seed(n + 3 * b + heads)
        c = heads * 64
        q = torch.randn(b, n, c, generator=g)
        k = torch.randn(b, 1, c, generator=g).expand(b, n, c)
        v = torch.randint(-8, 9, (b, 1, c), generator=g).float().expand(b, n, c)
        out = _launch_attention(torch.cat([q, k, v], -1).to(dtype), heads)
        assert torch.equal(out, v.to(dtype)), f"n={n} b={b} heads={heads}"


def test_vit_attention_refuses_other_head_dims():
    from etainv import _capi
    lib = _capi.load()
    x = torch.zeros(4096, dtype=torch.float16, device="cuda")
    assert lib.etainv_op_vit_attention(x.data_ptr(), x.data_ptr(), 1, 4, 1, 40, _capi.F16, None) != 0
    assert "head_dim 64" in lib.etainv_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------- head
def _launch_head(x, index, ln, proj):
    from etainv import _capi
    lib = _capi.load()
    b, n, d = x.shape
    dev = lambda t: None if t is None else t.cuda().contiguous()
    xd, idx, w = dev(x), dev(index), dev(proj)
    gamma, beta = (dev(ln[0]), dev(ln[1])) if ln else (None, None)
    out = torch.empty(b, proj.shape[0], dtype=torch.float32, device="cuda")
    _capi.check(lib.etainv_clip_embed_head(_capi.ptr(xd), _capi.dtype_code(x.dtype), _capi.ptr(idx), b, n, d, _capi.ptr(gamma), _capi.ptr(beta), 1e-5,
                                           _capi.ptr(w), _capi.dtype_code(proj.dtype), proj.shape[0], _capi.ptr(out), _capi.stream_ptr()))
    return out.cpu()


@pytest.mark.parametrize("with_ln", [True, False])
@pytest.mark.parametrize("p", [64, 512])
@pytest.mark.parametrize("d", [128, 768])
def test_embed_head(d, p, with_ln):
    g = torch.Generator().manual_seed(d + p)
    n = 7
    x = torch.randn(5, n, d, generator=g)
    index = torch.tensor([0, n - 1, n // 2, 0, n - 1], dtype=torch.int32)
    ln = (1 + 0.1 * torch.randn(d, generator=g), 0.05 * torch.randn(d, generator=g)) if with_ln else None
    proj = torch.randn(p, d, generator=g) * d ** -0.5
    ref = cr.head(x[torch.arange(5), index.long()], ln, proj)
    bound = 8 * EPS32 * math.sqrt(d)
    for b in (1, 5):
        out = _launch_head(x[:b], index[:b], ln, proj)
        err = (out.double() - ref[:b])
        print(f"clip-head d={d} P={p} ln={with_ln} B={b}: L2 {err.norm(dim=-1).max():.3e} max {err.abs().max():.3e} bound {bound:.3e}")
        assert err.norm(dim=-1).max() <= bound and err.abs().max() <= bound
    full = _launch_head(x, index, ln, proj)
    for r in range(5):
        alone = _launch_head(x[r:r + 1], index[r:r + 1], ln, proj)
        assert torch.equal(alone[0].view(torch.int32), full[r].view(torch.int32)), f"row {r} depends on B"
    if not with_ln:                                                   # no index array: token 0
        assert torch.equal(_launch_head(x, None, ln, proj), _launch_head(x, torch.zeros(5, dtype=torch.int32), ln, proj))


# ---------------------------------------------------------------------------------------------------------------- scores
@pytest.mark.parametrize("t", [1, 3])
@pytest.mark.parametrize("mode", cr.MODES)
def test_scores(mode, t):
    from metrics.clip_similarity import MODES, clip_similarity
    assert MODES == cr.MODES
    p = 64
    img_src, img_tgt = cr.unit_rows((4, p), 1), cr.unit_rows((4, p), 2)
    txt_src, txt_tgt = cr.unit_rows((4, t, p), 3), cr.unit_rows((4, t, p), 4)
    txt_src[3] = txt_tgt[3]                                           # an exact tie: acc is 0.0
    ref = cr.scores(mode, img_src, img_tgt, txt_src, txt_tgt)
    run = lambda sl: clip_similarity(cr.MODES.index(mode), img_src[sl].cuda(), img_tgt[sl].cuda(), txt_src[sl].cuda(), txt_tgt[sl].cuda()).cpu()
    full = run(slice(0, 4))
    assert full.dtype == torch.float32 and full.shape == (4,)
    if mode == "text_img_acc":
        assert torch.equal(full.double(), ref) and full[3] == 0.0
    else:
        assert (full.double() - ref).abs().max() <= 1e-6
    assert torch.equal(full.view(torch.int32), run(slice(0, 4)).view(torch.int32))
    for r in range(4):
        assert torch.equal(run(slice(r, r + 1)).view(torch.int32), full[r:r + 1].view(torch.int32)), f"pair {r} depends on B"
    # mode 4: all four scores of every pair in one launch, each bit-identical to its own mode's
    every = clip_similarity(4, img_src.cuda(), img_tgt.cuda(), txt_src.cuda(), txt_tgt.cuda()).cpu()
    assert every.shape == (4, 4) and torch.equal(every[:, cr.MODES.index(mode)].contiguous().view(torch.int32), full.view(torch.int32))


def test_scores_refuse_unknown_mode_and_no_templates():
    from etainv import _capi
    lib = _capi.load()
    e = torch.zeros(64, dtype=torch.float32, device="cuda")
    out = torch.zeros(1, dtype=torch.float32, device="cuda")
    assert lib.etainv_clip_similarity(e.data_ptr(), e.data_ptr(), e.data_ptr(), e.data_ptr(), 1, 1, 64, 5, out.data_ptr(), None) != 0
    assert "unknown metric mode" in lib.etainv_last_error().decode()
    assert lib.etainv_clip_similarity(e.data_ptr(), e.data_ptr(), e.data_ptr(), e.data_ptr(), 1, 0, 64, 0, out.data_ptr(), None) != 0
    assert "at least 1" in lib.etainv_last_error().decode()
