"""Per-op parity of the kernels the VAE and the CLIP text encoder launch (etainv/nets.py), in the forms they launch them:
etainv_op_conv3x3_ex (pad0, fused upsample, NCHW output), the two-slot GEMM at widths that are no multiple of 160, im2col, row softmax,
quick_gelu, embedding, causal attention, GroupNorm at 4 / 8 / 16 channels per group, LayerNorm at 768 -- each against a float64 reference built
from the SAME rounded inputs the kernel reads, and the blocks of nets.py against the oracle's modules in float64.

Every output is allocated with a guard region behind it (marker -777) and pre-filled with NaN: a write past the extent or an element left
unwritten fails.  No test asserts a global norm alone: GEMM-like ops are checked per 64 x 64 block (2 * TOL, the convention of
test_gemm_persistent_ring) and, for convs, on the four border lines of the output; norms per (image, group) / per row; attention per (batch, head)
and per query row.  Tolerances: TOL of tests/test_kernels_gpu.py (2e-3 fp16 / 1.2e-2 bf16 / 2e-5 fp32) on relative L2; elementwise kernels
against one ulp of the output type (r = 2^-10 / 2^-7 / 2^-20: fp32 arithmetic, one rounding)."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_kernels_gpu import TOL, capi, relerr, rnd  # noqa: F401  (capi: fixture)

pytestmark = pytest.mark.gpu

DTYPES3 = [torch.float16, torch.bfloat16, torch.float32]
R_ULP = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7, torch.float32: 2.0 ** -20}     # one ulp of the output type = 2 x the worst rounding
U_RND = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 0.0}            # worst relative error of one rounding to an io type
MARK = -777.0
GUARD_ROWS = 64


# ------------------------------------------------------------------------------------------------ helpers
def guarded_flat(n, dtype, guard):
    """n + guard elements: NaN where the kernel must write, the marker behind it"""
    buf = torch.full((n + guard,), float("nan"), dtype=dtype, device="cuda")
    buf[n:] = MARK
    return buf


def guarded(rows, cols, dtype):
    """[rows + 64][cols], the last 64 rows the guard"""
    return guarded_flat(rows * cols, dtype, GUARD_ROWS * cols).reshape(rows + GUARD_ROWS, cols)


def assert_guard(buf, rows):
    torch.cuda.synchronize()
    assert torch.equal(buf[rows:], torch.full_like(buf[rows:], MARK)), "the kernel wrote behind its output"
    assert torch.isfinite(buf[:rows]).all(), "the kernel left part of its output unwritten (or wrote a non-finite value)"


def last_plan(capi):
    """what launch_igemm chose for this thread's last launch (etainv_op_last_igemm_plan): route name (None: no launch, or a refused one), tile, K split,
    form (1: ppconv's dual-M kernel; the epilogue kind of a dual-N launch)"""
    import ctypes
    lib, v = capi.load(), (ctypes.c_int * 5)()
    assert lib.etainv_op_last_igemm_plan(v, 5) == 5
    name = lib.etainv_op_igemm_route_name(v[0])
    return dict(route=name.decode() if name else None, bm=v[1], bn=v[2], ksplit=v[3], form=v[4])


def two_slot(bm, bn, ksplit):
    return dict(route="two-slot", bm=bm, bn=bn, ksplit=ksplit, form=0)


FP32_PLAN = dict(route="fp32", bm=128, bn=128, ksplit=1, form=0)


def rel64(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def block_err(out, ref, bm=64, bn=64):
    """worst relative L2 over the bm x bn blocks of an [M][N] matrix (ragged last blocks count with the elements they have)"""
    d2, r2 = (out.double() - ref.double()) ** 2, ref.double() ** 2
    m, n = d2.shape
    pm, pn = (-m) % bm, (-n) % bn
    d2, r2 = F.pad(d2, (0, pn, 0, pm)), F.pad(r2, (0, pn, 0, pm))
    d2 = d2.reshape((m + pm) // bm, bm, (n + pn) // bn, bn).sum((1, 3))
    r2 = r2.reshape((m + pm) // bm, bm, (n + pn) // bn, bn).sum((1, 3))
    return float((d2 / r2.clamp_min(1e-300)).sqrt().max())


def border_errs(out_nhwc, ref_nhwc):
    """relative L2 of the first / last output row and column, each on its own"""
    lines = {"top": (slice(None), 0), "bottom": (slice(None), -1), "left": (slice(None), slice(None), 0), "right": (slice(None), slice(None), -1)}
    return {k: rel64(out_nhwc[ix], ref_nhwc[ix]) for k, ix in lines.items()}


# ------------------------------------------------------------------------------------------------ 1. etainv_op_conv3x3_ex
# Route table (16-bit types; fp32 operands leave launch_igemm for csrc/f32path.hip, one kernel, before the rule).
# Every case runs on the two-slot kernels (no width is a multiple of 160).  Tile and K split, the same for fp16 and bf16, are asserted after every launch
# from what the library reports (last_plan; CONV_PLANS below restates the last two columns):
#
#   case                                      M      N    K tiles    tile        ksplit
#   pad0   2 x  16 x  24  128 -> 128          192    128     18      64 x 64     3
#   pad0   1 x 256 x 384  128 -> 128        24576    128     18      128 x 128   2      (192 big tiles fill 384 of 512 slots: the rule splits K too)
#   pad0   1 x 256 x 528  128 -> 128        33792    128     18      128 x 128   1      (264 big tiles: 128 x 128 without split-K)
#   pad0   3 x  12 x  20  256 -> 256          180    256     36      64 x 64     9      (ragged M tile)
#   s1+res 2 x  64 x  48  512 -> 512         6144    512     72      128 x 128   2
#   s1+res 1 x 176 x 192  128 -> 128        33792    128     18      128 x 128   1
#   s1+res 2 x   8 x   8  512 -> 512          128    512     72      64 x 64     18     (the VAE mid block on an 8 x 8 latent)
#   s1+res 3 x  10 x  12  128 -> 256          360    256     18      64 x 64     3      (ragged M, cin != cout)
#   ups    1 x   8 x  12  512 -> 512          384    512     72      64 x 64     18
#   ups    2 x  32 x  48  256 -> 256        12288    256     36      128 x 128   2
#   ups    1 x  88 x  96  128 -> 128        33792    128     18      128 x 128   1
#   out_nchw (all 16 cases)               768 / 240    4   18 / 72   64 x 64     1      (out_nchw and split-K exclude each other)
#
# out_nchw: test_conv3x3_ex_out_nchw asserts 64 x 64, ksplit 1.
# So 128 x 128 without split-K, 128 x 128 with it, and 64 x 64 with split-K are each reached by a pad0, a stride-1 and an upsample case.  A
# 64 x 64 launch of a 3 x 3 conv WITHOUT split-K needs more than 512 small tiles and fewer than 192 big ones, which no VAE shape has: the NCHW
# cases and the short-K GEMMs of test_gemm_aux_shapes are the unsplit 64 x 64 launches.
# tests/test_kernels_gpu.py::test_split_k_small_m_deep_k in a run under ETAINV_TRACE_IGEMM=1: all four of its launches take the 64 x 64 tile with split-K
# (convs M = 64 / 256 / 256, N = 1280: ksplit 30 / 12 / 12; the GEMM (64, 1280, 5120): ksplit 20) -- 8 to 16 tiles of 128 x 160 are far from the
# 64 that `deep_k` asks for.  So split-K on 64 x 64 tiles was pinned before, for stride-1 convs at N = 1280 with a global norm; what is new here
# is that path under pad0 and the fused upsample, at N = 128 / 256 / 512, with a ragged M tile, and checked per block and on the border.
CONV_CASES = [
    ("pad0", 2, 16, 24, 128, 128), ("pad0", 1, 256, 384, 128, 128), ("pad0", 1, 256, 528, 128, 128), ("pad0", 3, 12, 20, 256, 256),
    ("s1", 2, 64, 48, 512, 512), ("s1", 1, 176, 192, 128, 128), ("s1", 2, 8, 8, 512, 512), ("s1", 3, 10, 12, 128, 256),
    ("ups", 1, 8, 12, 512, 512), ("ups", 2, 32, 48, 256, 256), ("ups", 1, 88, 96, 128, 128),
]
CONV_PLANS = dict(zip(CONV_CASES, [two_slot(64, 64, 3), two_slot(128, 128, 2), two_slot(128, 128, 1), two_slot(64, 64, 9),
                                   two_slot(128, 128, 2), two_slot(128, 128, 1), two_slot(64, 64, 18), two_slot(64, 64, 3),
                                   two_slot(64, 64, 18), two_slot(128, 128, 2), two_slot(128, 128, 1)]))


def conv_ref64(x, w, bias, mode):
    """x [b][cin][H][W], w [cout][cin][3][3] already rounded to the compute dtype; float64 on the host"""
    x, w, bias = x.double().cpu(), w.double().cpu(), bias.double().cpu()
    if mode == "pad0":
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, bias, stride=2, padding=0)
    if mode == "ups":
        return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, bias, padding=1)
    return F.conv2d(x, w, bias, padding=1)


def conv_ex(capi, x_nhwc, w_p, bias, res, out, b, h, wd, cin, cout, mode, dtype, out_nchw=0, io=0):
    stride, ups, pad0 = (2, 0, 1) if mode == "pad0" else (1, 1, 0) if mode == "ups" else (1, 0, 0)
    capi.check(capi.load().etainv_op_conv3x3_ex(capi.ptr(x_nhwc), capi.ptr(w_p), capi.ptr(bias), capi.ptr(res), capi.ptr(out), b, h, wd, cin, cout,
                                                stride, ups, pad0, out_nchw, io, capi.dtype_code(dtype), capi.stream_ptr()))


@pytest.mark.parametrize("dtype", DTYPES3)
@pytest.mark.parametrize("mode,b,h,wd,cin,cout", CONV_CASES)
def test_conv3x3_ex(capi, dtype, mode, b, h, wd, cin, cout):
    x = rnd(b, cin, h, wd, seed=1, dtype=dtype)
    w = rnd(cout, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5, dtype=dtype)
    bias = rnd(cout, seed=3)
    ref = conv_ref64(x, w, bias, mode).permute(0, 2, 3, 1).contiguous()                    # [b][Ho][Wo][cout]
    ho, wo = ref.shape[1], ref.shape[2]
    assert (ho, wo) == ((h // 2, wd // 2) if mode == "pad0" else (2 * h, 2 * wd) if mode == "ups" else (h, wd))
    m = b * ho * wo
    res = rnd(m, cout, seed=6, dtype=dtype) if mode == "s1" else None
    if res is not None:
        ref = ref + res.double().cpu().reshape(b, ho, wo, cout)
    out = guarded(m, cout, dtype)
    conv_ex(capi, x.permute(0, 2, 3, 1).contiguous(), w.permute(0, 2, 3, 1).contiguous(), bias, res, out, b, h, wd, cin, cout, mode, dtype)
    assert last_plan(capi) == (FP32_PLAN if dtype == torch.float32 else CONV_PLANS[(mode, b, h, wd, cin, cout)])
    assert_guard(out, m)
    got = out[:m].cpu()
    e_all, e_blk = relerr(got, ref.reshape(m, cout)), block_err(got, ref.reshape(m, cout))
    e_brd = border_errs(got.reshape(b, ho, wo, cout), ref)
    print(f"conv3x3_ex {mode} {b}x{h}x{wd} {cin}->{cout} {dtype}: rel L2 {e_all:.2e}, worst 64x64 block {e_blk:.2e}, border " +
          " ".join(f"{k} {v:.2e}" for k, v in e_brd.items()))
    assert e_all < TOL[dtype]
    assert e_blk < 2 * TOL[dtype]
    assert max(e_brd.values()) < 2 * TOL[dtype], e_brd


IO_TYPES = [(0, torch.float32), (1, torch.float16), (2, torch.bfloat16)]     # out_io_dtype code (etainv._capi F32 / F16 / BF16), torch type


@pytest.mark.parametrize("dtype", DTYPES3)
@pytest.mark.parametrize("out_nchw", [3, 4])
@pytest.mark.parametrize("h,wd", [(16, 24), (10, 12)])
@pytest.mark.parametrize("cin", [128, 512])
def test_conv3x3_ex_out_nchw(capi, dtype, out_nchw, h, wd, cin):
    """conv_out of the VAE: N = 4, the first out_nchw channels stored as planes [b][out_nchw][H*W] of the io type.  Each plane of each image
    on its own: TOL of the compute type, plus the one rounding to the io type (2^-11 fp16, 2^-8 bf16 -- a bound on the relative L2 that rounding
    adds) only where the io type is coarser than the compute type: TOL already holds the rounding to the compute type.  With out_nchw = 3 the buffer holds exactly b * 3 * HW elements plus the guard: a store of the fourth channel lands in
    the next image's first plane or in the guard."""
    b, hw = 2, h * wd
    x = rnd(b, cin, h, wd, seed=1, dtype=dtype)
    bias0 = rnd(4, seed=3)
    for zero3 in (False, True):
        w = rnd(4, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5, dtype=dtype)
        bias = bias0.clone()
        if zero3:                                                                   # as nets.py pads the decoder's 3-channel conv_out
            w[3], bias[3] = 0, 0
        ref = conv_ref64(x, w, bias, "s1")                                          # [b][4][H][W]
        for code, io in IO_TYPES:
            n_out = b * out_nchw * hw
            out = guarded_flat(n_out, io, 4 * hw)
            conv_ex(capi, x.permute(0, 2, 3, 1).contiguous(), w.permute(0, 2, 3, 1).contiguous(), bias, None, out, b, h, wd, cin, 4, "s1", dtype,
                    out_nchw=out_nchw, io=code)
            assert last_plan(capi) == (FP32_PLAN if dtype == torch.float32 else two_slot(64, 64, 1))      # (out_nchw and split-K exclude each other)
            torch.cuda.synchronize()
            assert torch.equal(out[n_out:], torch.full_like(out[n_out:], MARK)), "a plane beyond out_nchw was written"
            got = out[:n_out].cpu().reshape(b, out_nchw, h, wd)
            assert torch.isfinite(got).all()
            tol = TOL[dtype] + (U_RND[io] if U_RND[io] > U_RND[dtype] else 0.0)        # TOL already holds one rounding to the compute type
            for i in range(b):
                for c in range(out_nchw):
                    if zero3 and c == 3:
                        assert not got[i, c].any(), "zero weights and zero bias give a zero plane"
                        continue
                    e = rel64(got[i, c], ref[i, c])
                    assert e < tol, f"image {i} plane {c} (io {io}, zero3 {zero3}): {e:.2e} >= {tol:.2e}"


# ------------------------------------------------------------------------------------------------ 2. etainv_op_gemm at VAE and CLIP shapes
# (m, n, k, kind).  16-bit types (gemm_plan, asserted after every launch): 128 x 128 without split-K for (24576, 128, 64) and (6144, 512, 256) (192 big
# tiles each); 64 x 64 for all the others, unsplit except (1024, 512, 1024) (ksplit 4) and the two CLIP shapes with k = 3072 (ksplit 12): split-K needs
# k / 64 >= 16, so k = 512 and k = 768 (12 K tiles) do not split.
GEMM_CASES = [
    (2 * 16 * 24, 128, 64, "im2col"), (2 * 8 * 12, 512, 64, "im2col"), (24576, 128, 64, "im2col"),
    (64, 64, 512, "score"), (256, 256, 512, "score"), (1024, 1024, 512, "score"),
    (512, 64, 512, "vt"), (512, 1024, 512, "vt"),
    (64, 512, 64, "pv"), (256, 512, 256, "pv"), (1024, 512, 1024, "pv"),
    (360, 256, 128, "shortcut"), (6144, 512, 256, "shortcut"),
    (77, 2304, 768, "clip"), (231, 768, 768, "clip"), (231, 3072, 768, "clip"), (231, 768, 3072, "clip"), (77, 768, 3072, "clip"),
]


def gemm_plan(m, n, k):
    if (m, n, k) in ((24576, 128, 64), (6144, 512, 256)):
        return two_slot(128, 128, 1)
    return two_slot(64, 64, 4 if (m, n, k) == (1024, 512, 1024) else 12 if k == 3072 else 1)


@pytest.mark.parametrize("dtype", DTYPES3)
@pytest.mark.parametrize("m,n,k,kind", GEMM_CASES)
def test_gemm_aux_shapes(capi, dtype, m, n, k, kind):
    """a @ w.T in float64 (+ bias, + residual) per 64 x 64 block, with neither, either and both epilogue operands.  `score`: both operands are
    activations (Q K^T, unit scale); `pv`: A holds rows of a softmax (non-negative, sums 1, rounded to the dtype) and K = the row length"""
    lib = capi.load()
    if kind == "pv":
        a = (rnd(m, k, seed=1, scale=2.0).double() * 1.0).softmax(-1).to(dtype)
    else:
        a = rnd(m, k, seed=1, dtype=dtype)
    w = rnd(n, k, seed=2, scale=1.0 if kind == "score" else k ** -0.5, dtype=dtype)
    bias, res = rnd(n, seed=3), rnd(m, n, seed=4, dtype=dtype)
    prod = a.double() @ w.double().t()
    for use_b, use_r in ((False, False), (True, False), (False, True), (True, True)):
        ref = prod + (bias.double() if use_b else 0) + (res.double() if use_r else 0)
        out = guarded(m, n, dtype)
        capi.check(lib.etainv_op_gemm(capi.ptr(a), capi.ptr(w), capi.ptr(bias if use_b else None), capi.ptr(res if use_r else None), capi.ptr(out),
                                      m, n, k, 0, capi.dtype_code(dtype), capi.stream_ptr()))
        assert last_plan(capi) == (FP32_PLAN if dtype == torch.float32 else gemm_plan(m, n, k))
        assert_guard(out, m)
        e_all, e_blk = relerr(out[:m], ref), block_err(out[:m], ref)
        print(f"gemm {kind} ({m}, {n}, {k}) {dtype} bias {use_b} residual {use_r}: rel L2 {e_all:.2e}, worst 64x64 block {e_blk:.2e}")
        assert e_all < TOL[dtype]
        assert e_blk < 2 * TOL[dtype]


# ------------------------------------------------------------------------------------------------ 3. etainv_op_im2col3x3
def im2col_expected(x, cin):
    """x [rows][cin][H][W] float64 (already mixed where a premix applies): ([rows*H*W][64] with k = tap * cin + ci, zero elsewhere; mask of the
    (pixel, k) entries that are valid taps)"""
    rows, _, h, w = x.shape
    xp, ones = F.pad(x, (1, 1, 1, 1)), F.pad(torch.ones_like(x), (1, 1, 1, 1))
    out, valid = torch.zeros(rows, h, w, 64, dtype=torch.float64), torch.zeros(rows, h, w, 64, dtype=torch.bool)
    for t in range(9):
        ky, kx = t // 3, t % 3
        out[..., t * cin:(t + 1) * cin] = xp[:, :, ky:ky + h, kx:kx + w].permute(0, 2, 3, 1)
        valid[..., t * cin:(t + 1) * cin] = ones[:, :, ky:ky + h, kx:kx + w].permute(0, 2, 3, 1) > 0
    return out.reshape(-1, 64), valid.reshape(-1, 64)


def run_im2col(capi, x, cin, premix, dtype):
    rows, _, h, w = x.shape
    n = rows * h * w
    out = guarded(n, 64, dtype)
    capi.check(capi.load().etainv_op_im2col3x3(capi.ptr(x), capi.F32, cin, h, w, rows, capi.ptr(premix), capi.ptr(out), capi.dtype_code(dtype),
                                               capi.stream_ptr()))
    assert_guard(out, n)
    return out[:n]


@pytest.mark.parametrize("dtype", DTYPES3)
@pytest.mark.parametrize("rows,h,w", [(2, 16, 24), (3, 5, 7), (1, 64, 64)])
@pytest.mark.parametrize("cin", [3, 4])
def test_im2col3x3(capi, dtype, cin, rows, h, w):
    x = rnd(rows, cin, h, w, seed=1)                                                # fp32 NCHW, as nets.py passes it
    # without premix: a gather of the rounded input, bit for bit; zero for k >= 9 * cin and for every halo tap
    got = run_im2col(capi, x, cin, None, dtype).cpu()
    want, valid = im2col_expected(x.cpu().to(dtype).double(), cin)
    assert torch.equal(got.double(), want)
    assert not got[~valid].any()
    assert not valid[:, 9 * cin:].any() and valid[:, :9 * cin].any(0).all()
    # premix: [cin][cin + 1] = (matrix | bias), a NON-zero bias: it must not leak into the zero padding of the conv that follows
    pm = rnd(cin, cin + 1, seed=2)
    pm[:, cin] = torch.tensor([0.7, -1.3, 2.1, -0.4])[:cin].cuda()
    got = run_im2col(capi, x, cin, pm, dtype).cpu().double()
    x64, p64 = x.cpu().double(), pm.cpu().double()
    mix = torch.einsum("oc,rchw->rohw", p64[:, :cin], x64) + p64[:, cin][None, :, None, None]
    # magnitude that the fp32 mix rounds against: |bias| + sum |p x|.  cin + 1 fp32 operations, each within 2^-24 of its result (fused or not):
    # |fp32 mix - mix| <= (cin + 1) * 2^-24 * mag; then ONE rounding to the dtype (R_ULP is twice its worst case; 2^-25: half an fp16 subnormal step)
    mag = torch.einsum("oc,rchw->rohw", p64[:, :cin].abs(), x64.abs()) + p64[:, cin].abs()[None, :, None, None]
    want, valid = im2col_expected(mix, cin)
    slack, _ = im2col_expected(mag, cin)
    assert not got[~valid].any(), "halo taps and the columns behind 9 * cin stay exactly zero under a premix with bias"
    # (a purely relative bound cannot hold where the mix cancels to near zero: the fp32 error scales with `mag`, not with the result.)
    # Measured on an MI355X, worst |got - ref| / bound over all cases: 0.496 fp16, 0.498 bf16, 0.177 fp32 -- the 16-bit figure is the output
    # rounding itself (half of R_ULP), the dot-product term adds next to nothing to it
    bound = R_ULP[dtype] * want.abs() + (cin + 1) * 2.0 ** -24 * slack + 2.0 ** -25
    worst = float(((got - want).abs() / bound)[valid].max())
    print(f"im2col premix cin {cin} {rows}x{h}x{w} {dtype}: worst |got - ref| / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", DTYPES3)
@pytest.mark.parametrize("rows,h,w", [(2, 16, 24), (3, 5, 7)])
@pytest.mark.parametrize("decoder", [False, True])
def test_im2col_then_gemm_is_the_input_conv(capi, dtype, decoder, rows, h, w):
    """conv_in of the encoder (3 -> 128) and of the decoder (post_quant_conv 1x1, then 4 -> 512) as nets.py runs them: im2col (+ premix) and one
    K = 64 GEMM with _pack_conv_small weights, against F.conv2d(padding = 1) in float64 on the rounded input and weights; for the decoder against
    conv o 1 x 1 conv in float64 (the kernel rounds the mixed pixels to the dtype once more: inside TOL)"""
    from etainv.nets import _pack_conv_small
    cin, cout = (4, 512) if decoder else (3, 128)
    x = rnd(rows, cin, h, w, seed=1)
    w4 = rnd(cout, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5).to(dtype)
    bias = rnd(cout, seed=3)
    pm = None
    if decoder:
        pm = rnd(cin, cin + 1, seed=4, scale=0.5)
        pm[:, cin] = torch.tensor([0.7, -1.3, 2.1, -0.4]).cuda()
        x64 = F.conv2d(x.cpu().double(), pm[:, :cin].cpu().double()[:, :, None, None], pm[:, cin].cpu().double())
    else:
        x64 = x.cpu().to(dtype).double()
    ref = F.conv2d(x64, w4.cpu().double(), bias.cpu().double(), padding=1).permute(0, 2, 3, 1)      # [rows][h][w][cout]
    cols = run_im2col(capi, x, cin, pm, dtype).contiguous()
    wk = _pack_conv_small(w4.cpu().float()).to(dtype).cuda()
    m = rows * h * w
    out = guarded(m, cout, dtype)
    capi.check(capi.load().etainv_op_gemm(capi.ptr(cols), capi.ptr(wk), capi.ptr(bias), None, capi.ptr(out), m, cout, 64, 0, capi.dtype_code(dtype),
                                          capi.stream_ptr()))
    assert_guard(out, m)
    got = out[:m].cpu().reshape(rows, h, w, cout)
    e_all, e_brd = relerr(got, ref), border_errs(got, ref)
    print(f"im2col + gemm {'decoder' if decoder else 'encoder'} {rows}x{h}x{w} {dtype}: rel L2 {e_all:.2e}, border {e_brd}")
    assert e_all < TOL[dtype]
    assert max(e_brd.values()) < TOL[dtype], e_brd


# ------------------------------------------------------------------------------------------------ 4. etainv_op_row_softmax
@pytest.mark.parametrize("dtype", DTYPES3)
@pytest.mark.parametrize("gain", [1, 8, 40])
@pytest.mark.parametrize("n", [64, 200, 1024, 4096])
def test_row_softmax(capi, dtype, n, gain):
    """in place, scale 512^-0.5, against the float64 softmax of the rounded inputs: |got - ref| <= r * ref + 2^-24 elementwise, r one ulp of the
    output type (the kernel works in fp32 and rounds once).  Row 2 is constant, row 4 has one dominant entry"""
    rows, extra, scale = 7, 3, 512 ** -0.5
    g = torch.Generator().manual_seed(n + gain)
    x = torch.randn(rows + extra, n, generator=g) * gain * math.sqrt(512)
    x[2] = 3.0 * gain
    x[4, n // 3] = 2 * x[4].abs().max() + 50
    x = x.to(dtype)
    ref = (x[:rows].double() * scale).softmax(-1)
    buf = x.clone().cuda()
    capi.check(capi.load().etainv_op_row_softmax(capi.ptr(buf), rows, n, scale, capi.dtype_code(dtype), capi.stream_ptr()))
    torch.cuda.synchronize()
    buf = buf.cpu()
    assert torch.equal(buf[rows:], x[rows:]), "rows behind `rows` are untouched"
    got = buf[:rows].double()
    assert torch.isfinite(got).all()
    r = R_ULP[dtype]
    worst = float(((got - ref).abs() / (r * ref + 2.0 ** -24)).max())
    sums = got.sum(-1)
    print(f"row_softmax n {n} gain {gain} {dtype}: worst |got - ref| / (r ref + 2^-24) {worst:.3f}, row sums {float(sums.min()):.6f} .. {float(sums.max()):.6f}")
    assert worst <= 1.0
    assert float((sums - 1).abs().max()) <= r + n * 2.0 ** -24              # what the elementwise bound sums to
    if dtype != torch.float32:
        assert float((sums - 1).abs().max()) <= n * U_RND[dtype]


# ------------------------------------------------------------------------------------------------ 5. etainv_op_quick_gelu
@pytest.mark.parametrize("dtype", DTYPES3)
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("n", [1, 255, 257, 77 * 3072])
def test_quick_gelu(capi, dtype, n, inplace):
    """x * sigmoid(1.702 x) in float64 on the rounded input: |got - ref| <= r |ref| + 2^-24.  Half of x sweeps [-100, 100] (the fp32 exp
    overflows to inf at the negative end by design: the result is -0, never NaN), half is randn * 3"""
    g = torch.Generator().manual_seed(n)
    sweep = torch.linspace(-100, 100, (n + 1) // 2)
    x = torch.cat([sweep, torch.randn(n - sweep.numel(), generator=g) * 3]).to(dtype)
    ref = x.double() * torch.sigmoid(1.702 * x.double())
    src = torch.cat([x, torch.full((GUARD_ROWS,), MARK, dtype=dtype)]).cuda()
    dst = src if inplace else guarded_flat(n, dtype, GUARD_ROWS)
    capi.check(capi.load().etainv_op_quick_gelu(capi.ptr(src), capi.ptr(dst), n, capi.dtype_code(dtype), capi.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(dst[n:], torch.full_like(dst[n:], MARK))
    if not inplace:
        assert torch.equal(src[:n].cpu(), x), "the input of an out-of-place call is left alone"
    got = dst[:n].cpu().double()
    assert torch.isfinite(got).all()
    worst = float(((got - ref).abs() / (R_ULP[dtype] * ref.abs() + 2.0 ** -24)).max())
    print(f"quick_gelu n {n} inplace {inplace} {dtype}: worst |got - ref| / (r |ref| + 2^-24) {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ 6. etainv_op_embed
@pytest.mark.parametrize("dtype", DTYPES3)
@pytest.mark.parametrize("b", [1, 3])
def test_embed(capi, dtype, b):
    vocab, n_pos, d = 1000, 77, 768
    tok, pos = rnd(vocab, d, seed=1, scale=0.5, dtype=dtype), rnd(n_pos, d, seed=2, scale=0.5, dtype=dtype)
    ids = torch.randint(0, vocab, (b, n_pos), generator=torch.Generator().manual_seed(b))
    ids[:, 0], ids[:, 1], ids[:, 5], ids[:, 20:] = 0, vocab - 1, 0, vocab - 1       # both ends of the table, repeated
    out = guarded(b * n_pos, d, dtype)
    capi.check(capi.load().etainv_op_embed(capi.ptr(ids.cuda()), capi.ptr(tok), capi.ptr(pos), b, n_pos, d, capi.ptr(out), capi.dtype_code(dtype),
                                           capi.stream_ptr()))
    assert_guard(out, b * n_pos)
    want = (tok[ids.cuda()].float() + pos.float()[None]).to(dtype).reshape(b * n_pos, d)
    assert torch.equal(out[: b * n_pos], want)


# ------------------------------------------------------------------------------------------------ 7. etainv_op_causal_attention
def causal_attn(capi, qkv, b, n, heads, dtype, d=64):
    out = guarded(b * n, heads * d, dtype)
    capi.check(capi.load().etainv_op_causal_attention(capi.ptr(qkv), capi.ptr(out), b, n, heads, d, capi.dtype_code(dtype), capi.stream_ptr()))
    assert_guard(out, b * n)
    return out[: b * n]


@pytest.mark.parametrize("dtype", DTYPES3)
@pytest.mark.parametrize("gain", [1, 3])
@pytest.mark.parametrize("b,n,heads", [(1, 1, 1), (1, 2, 12), (3, 77, 12), (2, 80, 3)])
def test_causal_attention(capi, dtype, b, n, heads, gain):
    """float64 masked softmax attention (scale 0.125) per (batch, head) and per query row; gain 3 on q / k saturates the softmax (the online
    rescale works); causality bit for bit"""
    d, C = 64, heads * 64
    qkv32 = rnd(b, n, 3 * C, seed=1)
    qkv32[..., : 2 * C] *= gain
    qkv = qkv32.to(dtype)
    got = causal_attn(capi, qkv, b, n, heads, dtype).reshape(b, n, heads, d).permute(0, 2, 1, 3).double()      # [b][heads][n][d]
    q, k, v = (t.reshape(b, n, heads, d).permute(0, 2, 1, 3) for t in qkv.double().split(C, dim=-1))
    s = q @ k.transpose(-1, -2) * 0.125
    s = s.masked_fill(torch.ones(n, n, dtype=torch.bool, device=s.device).triu(1), float("-inf"))
    ref = s.softmax(-1) @ v
    e_bh = (got - ref).norm(dim=(2, 3)) / ref.norm(dim=(2, 3))
    e_row = (got - ref).norm(dim=3) / ref.norm(dim=3)
    print(f"causal attention b {b} n {n} heads {heads} gain {gain} {dtype}: worst (batch, head) {float(e_bh.max()):.2e}, worst query row {float(e_row.max()):.2e}")
    assert float(e_bh.max()) < TOL[dtype]
    assert float(e_row.max()) < 2 * TOL[dtype]
    # causality: another K and V at token j leaves every query i < j bit for bit, and changes query j (the new key is query j's own vector, so
    # that token j carries weight in query j's row in every head even where the softmax is saturated)
    j = n // 2
    qkv2 = qkv.clone()
    qkv2[:, j, C:2 * C] = qkv[:, j, :C]
    qkv2[:, j, 2 * C:] = rnd(b, C, seed=9, dtype=dtype)
    got1 = causal_attn(capi, qkv, b, n, heads, dtype).reshape(b, n, C)
    got2 = causal_attn(capi, qkv2, b, n, heads, dtype).reshape(b, n, C)
    assert torch.equal(got1[:, :j], got2[:, :j])
    for i in range(b):
        for h in range(heads):
            assert not torch.equal(got1[i, j, h * d:(h + 1) * d], got2[i, j, h * d:(h + 1) * d])


@pytest.mark.parametrize("dtype", DTYPES3)
@pytest.mark.parametrize("n,d", [(81, 64), (77, 32)])
def test_causal_attention_refuses_what_it_cannot_do(capi, dtype, n, d):
    b, heads = 1, 2
    qkv = rnd(b, n, 3 * heads * d, seed=1, dtype=dtype)
    out = torch.full((b * n, heads * d), MARK, dtype=dtype, device="cuda")
    with pytest.raises(capi.EtainvError):
        capi.check(capi.load().etainv_op_causal_attention(capi.ptr(qkv), capi.ptr(out), b, n, heads, d, capi.dtype_code(dtype), capi.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, MARK)), "a refused call launches nothing"


# ------------------------------------------------------------------------------------------------ 8. GroupNorm / LayerNorm at these widths
@pytest.mark.parametrize("dtype", DTYPES3)
@pytest.mark.parametrize("b,hw", [(1, 64), (2, 96), (3, 120), (2, 1024), (1, 16384)])
@pytest.mark.parametrize("c", [128, 256, 512])
def test_groupnorm_vae_widths(capi, dtype, c, b, hw):
    """32 groups of 4 / 8 / 16 channels (at C = 128 one 8-channel vector holds two groups), eps 1e-6, with and without SiLU.  Every channel
    carries its own offset ~ N(0, 2^2): statistics taken over the wrong channels are visibly wrong.  Per (image, group) against float64"""
    groups, eps = 32, 1e-6
    x = ((rnd(b, hw, c, seed=1) * 1.5 + 0.3) + 2.0 * rnd(c, seed=4)).to(dtype)
    gamma, beta = rnd(c, seed=2) * 0.1 + 1, rnd(c, seed=3) * 0.1
    base = F.group_norm(x.double().permute(0, 2, 1), groups, gamma.double(), beta.double(), eps).permute(0, 2, 1)      # [b][hw][c]
    scratch = torch.zeros(b * 65 * 64, dtype=torch.float32, device="cuda")
    for silu in (0, 1):
        ref = F.silu(base) if silu else base
        out = guarded(b * hw, c, dtype)
        capi.check(capi.load().etainv_op_groupnorm(capi.ptr(x), None, c, 0, capi.ptr(gamma), capi.ptr(beta), capi.ptr(out), b, hw, groups, eps, silu,
                                                   capi.ptr(scratch), capi.dtype_code(dtype), capi.stream_ptr()))
        assert_guard(out, b * hw)
        d = (out[: b * hw].double().reshape(b, hw, groups, c // groups) - ref.reshape(b, hw, groups, c // groups))
        e = d.norm(dim=(1, 3)) / ref.reshape(b, hw, groups, c // groups).norm(dim=(1, 3))                              # [b][groups]
        print(f"groupnorm C {c} b {b} hw {hw} silu {silu} {dtype}: worst (image, group) {float(e.max()):.2e}")
        assert float(e.max()) < 2 * TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES3)
@pytest.mark.parametrize("rows", [77, 231])
def test_layernorm_clip_width(capi, dtype, rows):
    c, eps = 768, 1e-5
    x = (rnd(rows, c, seed=1) * 1.5 + 0.3).to(dtype)
    gamma, beta = rnd(c, seed=2) * 0.1 + 1, rnd(c, seed=3) * 0.1
    out = guarded(rows, c, dtype)
    capi.check(capi.load().etainv_op_layernorm(capi.ptr(x), capi.ptr(gamma), capi.ptr(beta), capi.ptr(out), rows, c, eps, capi.dtype_code(dtype),
                                               capi.stream_ptr()))
    assert_guard(out, rows)
    ref = F.layer_norm(x.double(), (c,), gamma.double(), beta.double(), eps)
    e = (out[:rows].double() - ref).norm(dim=1) / ref.norm(dim=1)
    print(f"layernorm rows {rows} {dtype}: worst row {float(e.max()):.2e}")
    assert float(e.max()) < 2 * TOL[dtype]
    assert relerr(out[:rows], ref) < TOL[dtype]


# ------------------------------------------------------------------------------------------------ 9. blocks of nets.py against the oracle's modules
_vae = {}


def native_vae(dtype):
    from etainv.nets import NativeVAE
    if dtype not in _vae:
        _vae[dtype] = NativeVAE(None, dtype, 0)
    return _vae[dtype]


def oracle_vae64():
    if "oracle" not in _vae:
        from oracle.vae import build_vae
        _vae["oracle"] = build_vae(0).double()
    return _vae["oracle"]


def oracle_module(mod, dtype):
    """float64 copy of an oracle module whose conv / linear weights carry the rounding nets.py gives them (norm parameters and biases stay fp32)"""
    m = copy.deepcopy(mod)
    with torch.no_grad():
        for p in m.parameters():
            if p.ndim >= 2:
                p.copy_(p.float().to(dtype).double())
    return m


def block_input(b, c, h, w, dtype, seed=1):
    x = rnd(b, c, h, w, seed=seed, dtype=dtype)
    return x.permute(0, 2, 3, 1).contiguous(), x.double().cpu()                     # NHWC for nets.py, NCHW float64 for the oracle


def assert_block(got_nhwc, ref_nchw, dtype, what):
    """TOL per image and per 32-channel slice"""
    got, ref = got_nhwc.double().cpu().permute(0, 3, 1, 2), ref_nchw
    assert got.shape == ref.shape
    b, c = ref.shape[:2]
    d = (got - ref).reshape(b, c // 32, -1).norm(dim=2) / ref.reshape(b, c // 32, -1).norm(dim=2)
    print(f"{what} {dtype}: worst (image, 32-channel slice) {float(d.max()):.2e}, whole {rel64(got, ref):.2e}")
    assert torch.isfinite(got).all()
    assert float(d.max()) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES3)
@pytest.mark.parametrize("which", ["512->512", "128->256"])
def test_vae_res_block_vs_oracle(dtype, which):
    nat, ora = native_vae(dtype), oracle_vae64()
    if which == "512->512":
        r, mod, cin = nat.enc["mid"][0], ora.encoder.mid_block.resnets[0], 512
    else:
        r, mod, cin = nat.enc["down"][1]["res"][0], ora.encoder.down_blocks[1].resnets[0], 128                          # with its 1 x 1 shortcut
    x, x64 = block_input(2, cin, 8, 12, dtype)
    with torch.no_grad():
        ref = oracle_module(mod, dtype)(x64)
    assert_block(nat._run_res(r, x), ref, dtype, f"res block {which} 2x8x12")


@pytest.mark.parametrize("dtype", DTYPES3)
@pytest.mark.parametrize("h,w", [(8, 8), (8, 16)])
def test_vae_attention_block_vs_oracle(dtype, h, w):
    nat, ora = native_vae(dtype), oracle_vae64()
    x, x64 = block_input(2, 512, h, w, dtype)
    with torch.no_grad():
        ref = oracle_module(ora.encoder.mid_block.attentions[0], dtype)(x64)
    assert_block(nat._run_attn(nat.enc["mid"][1], x), ref, dtype, f"attention block 2x{h}x{w}")


@pytest.mark.parametrize("dtype", DTYPES3)
@pytest.mark.parametrize("level", [0, 2])
def test_vae_downsampler_vs_oracle(dtype, level):
    nat, ora = native_vae(dtype), oracle_vae64()
    c = (128, 256, 512)[level]
    x, x64 = block_input(2, c, 8, 12, dtype)
    with torch.no_grad():
        ref = oracle_module(ora.encoder.down_blocks[level].downsamplers[0].conv, dtype)(F.pad(x64, (0, 1, 0, 1)))
    assert_block(nat.ops.conv3(x, *nat.enc["down"][level]["down"], stride=2, pad0=1), ref, dtype, f"downsampler {c} 2x8x12")


@pytest.mark.parametrize("dtype", DTYPES3)
@pytest.mark.parametrize("level", [0, 2])
def test_vae_upsampler_vs_oracle(dtype, level):
    nat, ora = native_vae(dtype), oracle_vae64()
    c = (512, 512, 256)[level]
    x, x64 = block_input(2, c, 8, 12, dtype)
    with torch.no_grad():
        ref = oracle_module(ora.decoder.up_blocks[level].upsamplers[0].conv, dtype)(F.interpolate(x64, scale_factor=2.0, mode="nearest"))
    assert_block(nat.ops.conv3(x, *nat.dec["up"][level]["up"], ups=1), ref, dtype, f"upsampler {c} 2x8x12")
