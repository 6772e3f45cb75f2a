"""The two kernels of the plug-and-play editor in isolation: self-attention mode 3 (rows [u_s, u_t, c_t] x n_img: rows >= n_img take Q and K of row
r % n_img, V stays their own) on every route of csrc/self_attn_route.h and in the fp32-operand kernel, and etainv_op_rows_broadcast (the feature
injection: rows >= n_src become copies of row r % n_src)."""
import pytest
import torch

from etainv import _capi as capi
from tests import attention_ref as AR

pytestmark = pytest.mark.gpu
HEADS = 8
HALF = [torch.float16, torch.bfloat16]
# (d, N, n_img, route): one case per route; 528 / 576 items are >= two per CU on 256 CUs, the threshold of the persistent kernels
ROUTE_CASES = [(40, 64, 2, "d40-two-block"), (40, 256, 2, "d40-one-block-per-wave"), (40, 1024, 11, "d40-persistent"), (80, 64, 2, "d80"),
               (80, 1024, 6, "d80-persistent"), (160, 16, 2, "d160"), (160, 256, 2, "d160")]


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def pnp_maps(b, n_img):
    src = torch.arange(b) % n_img
    return src, src.clone(), torch.arange(b)


def injected_copy(qkv, n_img, d):
    """Q and K of rows >= n_img overwritten with those of row r % n_img: what mode 3 reads, as a tensor mode 0 can read"""
    out = qkv.clone()
    c2 = 2 * HEADS * d
    out[n_img:, :, :c2] = qkv[torch.arange(n_img, qkv.shape[0], device=qkv.device) % n_img][:, :, :c2]
    return out


def launch(qkv, b, n, d, mode, n_img, form="op", first_row=0, out=None):
    """form: "op" = etainv_op_self_attention; "rows" / "planes" = etainv_op_self_attention_ex on rows [b][n][3 C] with the scale applied by the kernel /
    on head-major planes with pre-scaled queries (the form the engine launches at head_dim 40 / 80); qkv is always given as plain rows"""
    lib = capi.load()
    dt = capi.dtype_code(qkv.dtype)
    out = torch.empty(b, n, HEADS * d, dtype=qkv.dtype, device="cuda") if out is None else out
    if form == "op":
        rc = lib.etainv_op_self_attention(capi.ptr(qkv), capi.ptr(out), b, n, HEADS, d, mode, n_img, dt, capi.stream_ptr())
    elif form == "rows":
        rc = lib.etainv_op_self_attention_ex(capi.ptr(qkv), capi.ptr(out), b, n, HEADS, d, mode, n_img, 0, first_row, 0, dt, capi.stream_ptr())
    else:
        planes = AR.to_head_major(AR.prescale_q(qkv, HEADS, d), HEADS).contiguous()
        rc = lib.etainv_op_self_attention_ex(capi.ptr(planes), capi.ptr(out), b, n, HEADS, d, mode, n_img, 1, first_row, 1, dt, capi.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


def relerr(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("d,n,n_img,route", ROUTE_CASES)
def test_mode3_equals_mode0_on_injected_copy_bitwise(dtype, d, n, n_img, route):
    """same shape, same route, same arithmetic: bit for bit, in every form the launcher takes; rows < n_img are those of the plain launch on the
    untouched tensor, rows >= n_img are not"""
    b = 3 * n_img
    assert AR.self_attention_route(b, n, HEADS, d, n_cu()) == route
    qkv = AR.random_qkv(b, n, HEADS, d, dtype, seed=d + n).cuda()
    copy = injected_copy(qkv, n_img, d)
    for form in ("op",) + (("rows", "planes") if d in (40, 80) else ()):
        rc, got = launch(qkv, b, n, d, 3, n_img, form)
        assert rc == 0, capi.load().etainv_last_error()
        rc, want = launch(copy, b, n, d, 0, 1, form)
        assert rc == 0
        assert torch.equal(got, want), (form, relerr(got, want))
        rc, plain = launch(qkv, b, n, d, 0, 1, form)
        assert rc == 0 and torch.equal(got[:n_img], plain[:n_img])
        e = relerr(got[n_img:], plain[n_img:])
        print(f"mode 3 vs mode 0, {route} {form} {dtype}: rows >= n_img differ by rel L2 {e:.2e}")
        assert e > 1e-2


@pytest.mark.parametrize("dtype", HALF + [torch.float32])
@pytest.mark.parametrize("d,n,n_img,route", ROUTE_CASES)
def test_mode3_vs_float64(dtype, d, n, n_img, route):
    """softmax(Q_s K_s^T) V_own in float64, at the three bounds (global, worst 32-query block, worst query) the mode 1 / 2 tests of
    tests/test_kernels_gpu.py hold that head_dim to; torch.float32 is the fp32-operand kernel of csrc/f32path.hip"""
    b = 3 * n_img
    if dtype == torch.float32 and n_img > 2:
        n_img, b = 2, 6                                          # (the fp32 kernel has one route: the item counts of the persistent cases mean nothing to it)
    qkv = AR.random_qkv(b, n, HEADS, d, dtype, seed=d + n + 1).cuda()
    rc, out = launch(qkv, b, n, d, 3, n_img)
    assert rc == 0, capi.load().etainv_last_error()
    assert torch.isfinite(out).all()
    ref = AR.ref_self_attention(qkv, HEADS, *pnp_maps(b, n_img), dt=torch.float64)
    AR.check_attention(out, ref, HEADS, d, dtype, 1.0, f"pnp mode 3 route={route if dtype != torch.float32 else 'fp32'}")
    if dtype == torch.float32:                                   # ... and the bitwise pair on that kernel
        rc, want = launch(injected_copy(qkv, n_img, d), b, n, d, 0, 1)
        assert rc == 0 and torch.equal(out, want)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_mode3_refusals_launch_nothing(dtype):
    """a row count that is not 3 n_img, a first_row, n_img = 0: non-zero status, the layout named in the message, the output untouched"""
    lib = capi.load()
    d, n, n_img = 40, 64, 2
    qkv = AR.random_qkv(4 * n_img, n, HEADS, d, dtype, seed=3).cuda()
    sentinel = torch.full((4 * n_img, n, HEADS * d), 7.0, dtype=dtype, device="cuda")
    for b, img, first_row in ((4 * n_img, n_img, 0), (3 * n_img, n_img, n_img), (3 * n_img, n_img, -1), (3 * n_img, 0, 0)):
        out = sentinel.clone()
        rc, _ = launch(qkv, b, n, d, 3, img, "rows", first_row, out=out)
        assert rc != 0 and "[u_s, u_t, c_t]" in lib.etainv_last_error().decode(), (b, img, first_row)
        assert torch.equal(out, sentinel)
    out = sentinel.clone()
    rc, _ = launch(qkv, 3 * n_img, n, d, 4, n_img, out=out)      # and there is no mode 4
    assert rc != 0 and torch.equal(out, sentinel)


# ----------------------------------------------------------------------------------------------------------------- row broadcast
def broadcast(x, rows, n_src, row_elems, dtype_code=None):
    rc = capi.load().etainv_op_rows_broadcast(capi.ptr(x), rows, n_src, row_elems, capi.dtype_code(x.dtype) if dtype_code is None else dtype_code,
                                              capi.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n_src", [1, 2, 3])
@pytest.mark.parametrize("row_elems", [40, 4 * 1280, 16 * 1280])      # 80 bytes (less than one block's stride), the engine's rows at L = 8 and L = 16
def test_rows_broadcast_equals_indexing(dtype, n_src, row_elems):
    rows = 3 * n_src
    g = torch.Generator().manual_seed(row_elems + n_src)
    x = torch.randn(rows + 1, row_elems, generator=g).to(dtype).cuda()                     # (+ a guard row behind the activation)
    want = x.clone()
    want[:rows] = x[torch.arange(rows, device="cuda") % n_src]
    assert broadcast(x, rows, n_src, row_elems) == 0, capi.load().etainv_last_error()
    assert torch.equal(x.view(torch.uint8), want.view(torch.uint8))                        # source rows and the guard row untouched, the rest copies


def test_rows_broadcast_refusals():
    lib = capi.load()
    x = torch.randn(6, 48, generator=torch.Generator().manual_seed(1)).half().cuda()
    keep = x.clone()
    for args in ((6, 2, 41), (6, 2, 47), (6, 4, 48), (6, 0, 48), (0, 2, 48)):              # 82- and 94-byte rows (2 and 14 bytes over), rows % n_src, empty
        assert broadcast(x, *args) != 0 and "rows_broadcast" in lib.etainv_last_error().decode(), args
    assert lib.etainv_op_rows_broadcast(None, 6, 2, 48, capi.F16, capi.stream_ptr()) != 0 and "null" in lib.etainv_last_error().decode()
    assert broadcast(x, 6, 2, 48, dtype_code=7) != 0
    assert torch.equal(x, keep)
    assert broadcast(x, 2, 2, 48) == 0 and torch.equal(x, keep)                             # nothing to overwrite
