"""The attention kernels in the forms the engine launches them: pre-scaled queries (q_prescaled = 1 at head_dim 40 / 80), head-major QKV planes, the three-row
layouts (first_row = n_img, first_row < 0), at the shapes that reach each kernel route -- through etainv_op_self_attention_ex / etainv_op_gemm_ln_hm.
References and bounds: tests/attention_ref.py (checked on the CPU by tests/test_attention_ref.py).  Which route a launch takes is decided from the dispatch
rules and the device's CU count (AR.self_attention_route) and asserted as the premise of each case."""
import ctypes as C

import pytest
import torch

from tests import attention_ref as AR

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
TOL = AR.TOL


@pytest.fixture(scope="module")
def capi():
    from etainv import _capi
    _capi.load()
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _capi


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


SENTINEL = 7.0


def attn_status(capi, x, b, n, heads, d, mode=0, n_img=1, pre=0, first_row=0, hm=0):
    """(status, out): out is pre-filled with SENTINEL so that a launch that must not happen can be seen not to have happened"""
    lib = capi.load()
    out = torch.full((b, n, heads * d), SENTINEL, dtype=x.dtype, device="cuda")
    st = lib.etainv_op_self_attention_ex(capi.ptr(x), capi.ptr(out), b, n, heads, d, mode, n_img, pre, first_row, hm, capi.dtype_code(x.dtype), capi.stream_ptr())
    torch.cuda.synchronize()
    return st, out


def attn(capi, x, b, n, heads, d, **kw):
    st, out = attn_status(capi, x, b, n, heads, d, **kw)
    capi.check(st)
    return out


def both_layouts(capi, qkv, heads, d, **kw):
    """row-major and head-major calls on the same values: only the layout of an intermediate changes -> equal bits.  Returns the head-major call's output."""
    b, n, _ = qkv.shape
    rm = attn(capi, qkv, b, n, heads, d, hm=0, **kw)
    hm = attn(capi, AR.to_head_major(qkv, heads), b, n, heads, d, hm=1, **kw)
    assert torch.equal(hm, rm), f"head-major and row-major calls differ in {int((hm != rm).any(-1).sum())} token rows"
    return hm


def check(out, qkv, heads, d, maps=(None, None, None), pre=True, label=""):
    assert torch.isfinite(out).all()
    ref = AR.ref_self_attention(qkv, heads, *maps, prescaled=pre)
    route = AR.self_attention_route(qkv.shape[0], qkv.shape[1], heads, d, n_cu())
    AR.check_attention(out, ref, heads, d, qkv.dtype, 1.0, f"{label} route={route} prescaled={int(pre)}",
                       emulate=lambda: AR.emulate_16bit(qkv, heads, *maps, prescaled=pre))
    return ref


# --------------------------------------------------------------------------------------------------------- a. engine form = test form
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,n,b,heads,route", [
    (40, 4096, 1, 8, "d40-one-block-per-wave"),    # 128 blocks
    (40, 4096, 4, 8, "d40-two-block"),             # 256 items: below two per CU
    (40, 4096, 16, 8, "d40-persistent"),           # 1024 items
    (40, 4096, 9, 8, "d40-persistent"),            # 576 items: uneven
    (80, 1024, 4, 8, "d80"),                       # 128 items
    (80, 1024, 16, 8, "d80-persistent"),           # 512 items
    (80, 1024, 33, 4, "d80-persistent"),           # 528 items, b * heads % 8 != 0: the item order without the XCD remap
    (160, 256, 4, 8, "d160"),
])
def test_self_attention_engine_form(capi, dtype, d, n, b, heads, route):
    """One launch per kernel route as the UNet makes it (scale * log2 e already in Q; head-major planes where the kernel reads them) against the fp32 reference of
    the rounded q', and the same bits from the row-major call."""
    assert AR.self_attention_route(b, n, heads, d, n_cu()) == route, f"{n_cu()} CUs: this shape no longer reaches the {route} kernel"
    qkv = AR.random_qkv(b, n, heads, d, dtype, seed=n + b + d)
    if d == 160:      # the scale stays in the kernel, rows only
        out = attn(capi, qkv.cuda(), b, n, heads, d)
        check(out, qkv.cuda(), heads, d, pre=False, label="engine_form")
        return
    qkv = AR.prescale_q(qkv, heads, d).cuda()
    out = both_layouts(capi, qkv, heads, d, pre=1)
    check(out, qkv, heads, d, label="engine_form")


# --------------------------------------------------------------------------------------------------------- b. the 768 x 768 configuration's launches
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,n,b", [(40, 9216, 8), (40, 9216, 16), (80, 2304, 8), (80, 2304, 11)])
def test_self_attention_config5_launches(capi, dtype, d, n, b):
    """96^2 = 9216 and 48^2 = 2304 tokens on the persistent kernels (1152 / 2304 and 576 / 792 items: 4.5, 9, 2.25 and ~3.1 per block on 256 CUs), both layouts,
    pre-scaled.  The fp32 reference runs on the device one batch row at a time (a row's scores are 2.7 GB at N = 9216)."""
    heads = 8
    assert AR.self_attention_route(b, n, heads, d, n_cu()) == f"d{d}-persistent"
    qkv = AR.prescale_q(AR.random_qkv(b, n, heads, d, dtype, seed=n + b), heads, d).cuda()
    out = both_layouts(capi, qkv, heads, d, pre=1)
    check(out, qkv, heads, d, label="config5")


# --------------------------------------------------------------------------------------------------------- c. row layouts through the persistent kernels
FORMS = [(1, 0), (2, 0), (1, 8), (1, -1)]     # (mode, first_row) at n_img = 8


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,n", [(80, 1024), (40, 2048)])
def test_self_attention_row_layouts_persistent(capi, dtype, d, n):
    """n_img = 8: prompt-to-prompt and MasaCtrl couplings on all 32 rows, and prompt-to-prompt on the two 24-row layouts, in both QKV layouts -- against row_maps +
    the fp32 reference, and every row of a three-row call equal, bit for bit, to its row of the four-row call (the persistent kernel on both sides)."""
    n_img, heads = 8, 8
    qkv4 = AR.prescale_q(AR.random_qkv(4 * n_img, n, heads, d, dtype, seed=n + d), heads, d).cuda()
    outs = {}
    for mode, first_row in FORMS:
        b = 4 * n_img if first_row == 0 else 3 * n_img
        assert AR.self_attention_route(b, n, heads, d, n_cu()) == f"d{d}-persistent"
        x = qkv4 if first_row == 0 else qkv4[AR.rows_in_four_row_call(n_img, first_row).cuda()].contiguous()
        out = both_layouts(capi, x, heads, d, mode=mode, n_img=n_img, pre=1, first_row=first_row)
        check(out, x, heads, d, AR.row_maps(b, n_img, mode, first_row), label=f"row_layouts mode={mode} first_row={first_row}")
        outs[mode, first_row] = out
    for first_row in (n_img, -1):
        in4 = AR.rows_in_four_row_call(n_img, first_row).cuda()
        same = (outs[1, first_row] == outs[1, 0][in4]).flatten(1).all(1)
        assert bool(same.all()), f"first_row={first_row}: rows {(~same).nonzero().flatten().tolist()} differ from the four-row call"


@pytest.mark.parametrize("dtype", DTYPES)
def test_self_attention_rejected_forms_launch_nothing(capi, dtype):
    lib = capi.load()
    n_img, heads, n = 2, 8, 256
    def rejected(x, b, d, **kw):
        st, out = attn_status(capi, x, b, n, heads, d, **kw)
        assert st != 0 and len(lib.etainv_last_error()) > 0
        assert bool((out == SENTINEL).all()), "a rejected call wrote to its output"
    x3 = AR.random_qkv(3 * n_img, n, heads, 80, dtype, 1).cuda()
    rejected(x3, 3 * n_img, 80, mode=2, n_img=n_img, first_row=n_img)          # MasaCtrl needs all four roles
    rejected(x3, 3 * n_img, 80, mode=2, n_img=n_img, first_row=-1)
    rejected(AR.random_qkv(4 * n_img, n, heads, 80, dtype, 1).cuda(), 4 * n_img, 80, mode=1, n_img=n_img, first_row=n_img)   # row count of another layout
    x160 = AR.random_qkv(2, n, heads, 160, dtype, 2).cuda()
    rejected(AR.to_head_major(x160, heads), 2, 160, hm=1)                       # no head-major reader at head_dim 160
    rejected(x160, 2, 160, pre=1)                                               # ... and no pre-scaled queries
    x32 = AR.random_qkv(2, n, heads, 40, torch.float32, 3).cuda()
    rejected(AR.to_head_major(x32, heads), 2, 40, hm=1)                         # fp32 path: rows only, scale in the kernel
    rejected(x32, 2, 40, pre=1)
    st, out = attn_status(capi, x32, 2, n, heads, 40)                           # (the accepted fp32 call next to them)
    assert st == 0 and not bool((out == SENTINEL).any())


# --------------------------------------------------------------------------------------------------------- d. the item decoder, made visible
@pytest.mark.parametrize("hm", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,n", [(80, 1024), (40, 2048)])
def test_self_attention_item_decoder_coded_inputs(capi, dtype, d, n, hm):
    """Tolerances cannot tell `slightly wrong` from `wrong row`; coded inputs can (AR.coded_v_qkv / AR.coded_qk_qkv: inputs exact in 16 bits whose outputs carry, as
    signs, the id of the (row, head) the values came from / of the key token that owns the softmax).  n_img = 8, modes 0 / 1 / 2 and the two three-row forms."""
    n_img, heads = 8, 8
    for mode, first_row in [(0, 0)] + FORMS:
        b = 4 * n_img if first_row == 0 else 3 * n_img
        assert AR.self_attention_route(b, n, heads, d, n_cu()) == f"d{d}-persistent"
        qm, km, vm = AR.row_maps(b, n_img, mode, first_row)
        kw = dict(mode=mode, n_img=n_img if mode else 1, pre=1, first_row=first_row, hm=hm)
        lay = (lambda t: AR.to_head_major(t, heads)) if hm else (lambda t: t)
        # V source
        x = AR.prescale_q(AR.coded_v_qkv(b, n, heads, d, dtype, seed=mode + 3), heads, d).cuda()
        got = AR.decode_v_ids(attn(capi, lay(x), b, n, heads, d, **kw), heads, d).cpu()
        want = AR.expected_v_ids(vm, n, heads)
        bad = (got != want).nonzero()
        assert len(bad) == 0, f"mode={mode} first_row={first_row}: V of (row, query, head) {bad[0].tolist()} came from id {int(got[tuple(bad[0])])}, expected {int(want[tuple(bad[0])])}"
        # Q and K source
        x = AR.prescale_q(AR.coded_qk_qkv(b, n, heads, d, dtype), heads, d).cuda()
        out = attn(capi, lay(x), b, n, heads, d, **kw)
        assert torch.isfinite(out).all()
        got = AR.decode_tokens(out, heads, d).cpu()
        want = AR.expected_tokens(qm, km, n, heads)
        bad = (got != want).nonzero()
        assert len(bad) == 0, f"mode={mode} first_row={first_row}: (row, query, head) {bad[0].tolist()} attended token {int(got[tuple(bad[0])])}, expected {int(want[tuple(bad[0])])}"


# --------------------------------------------------------------------------------------------------------- e. producer -> consumer on planes
def _folded_projection(capi, dtype, m, n_out, k):
    """operands of a LayerNorm-consumer GEMM (the recipe of test_kernels_gpu.py): raw rows, their (mean, rstd), folded weights and vectors"""
    lib = capi.load()
    g = torch.Generator().manual_seed(11)
    x = ((torch.randn(m, k, generator=g) * 1.5).to(dtype) + 0.3).cuda()
    xf = x.float()
    stat = torch.stack([xf.mean(-1), (xf.var(-1, unbiased=False) + 1e-5).rsqrt()], 1).contiguous()
    r = lambda *s, seed: torch.randn(*s, generator=torch.Generator().manual_seed(seed)).cuda()
    w = r(n_out, k, seed=5) * k ** -0.5
    gamma, beta, bias = 1.0 + 0.3 * r(k, seed=6), 0.2 * r(k, seed=7), r(n_out, seed=8)
    wp = torch.empty(n_out, k, dtype=dtype, device="cuda")
    s_vec, c_vec = torch.empty(n_out, device="cuda"), torch.empty(n_out, device="cuda")
    capi.check(lib.etainv_op_ln_fold(capi.ptr(w), capi.ptr(gamma), capi.ptr(beta), capi.ptr(bias), n_out, k, 0, 1.0, capi.ptr(wp), capi.ptr(s_vec), capi.ptr(c_vec),
                                     capi.dtype_code(dtype), capi.stream_ptr()))
    return x, stat, wp, s_vec, c_vec


def _qkv_projections(capi, ops, dtype, m, n_out, k, heads, d, tokens):
    """(row-major output of etainv_op_gemm_ln, output buffer of etainv_op_gemm_ln_hm, wrote_head_major)"""
    lib = capi.load()
    x, stat, wp, s_vec, c_vec = ops
    dt = capi.dtype_code(dtype)
    rows = torch.full((m, n_out), float("nan"), dtype=dtype, device="cuda")
    capi.check(lib.etainv_op_gemm_ln(capi.ptr(x), capi.ptr(wp), capi.ptr(c_vec), capi.ptr(s_vec), capi.ptr(stat), None, capi.ptr(rows), None, None, m, n_out, k, 0, dt,
                                     capi.stream_ptr()))
    buf = torch.full((m * n_out,), float("nan"), dtype=dtype, device="cuda")
    wrote = C.c_int(-1)
    capi.check(lib.etainv_op_gemm_ln_hm(capi.ptr(x), capi.ptr(wp), capi.ptr(c_vec), capi.ptr(s_vec), capi.ptr(stat), capi.ptr(buf), m, n_out, k, heads, d, tokens,
                                        C.byref(wrote), dt, capi.stream_ptr()))
    torch.cuda.synchronize()
    return rows, buf, wrote.value


@pytest.mark.parametrize("dualn", ["1", "0"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b,tokens,d", [(16, 4096, 40), (16, 1024, 80), (8, 9216, 40), (8, 2304, 80)])
def test_qkv_projection_planes_feed_the_attention_kernel(capi, dtype, monkeypatch, b, tokens, d, dualn):
    """The fused QKV projection writes the planes (dual-N kernel, and the ring kernel with ETAINV_DUALN=0) and the persistent attention kernel reads them: the planes
    hold exactly the row-major projection's values, and attention on them gives exactly the row-major pair's output."""
    monkeypatch.setenv("ETAINV_DUALN", dualn)
    heads = 8
    m, n_out, k = b * tokens, 3 * heads * d, heads * d
    assert AR.self_attention_route(b, tokens, heads, d, n_cu()) == f"d{d}-persistent"
    ops = _folded_projection(capi, dtype, m, n_out, k)
    rows, buf, wrote = _qkv_projections(capi, ops, dtype, m, n_out, k, heads, d, tokens)
    assert wrote == 1
    assert torch.isfinite(rows).all() and torch.isfinite(buf).all()
    qkv = rows.reshape(b, tokens, n_out)
    assert torch.equal(AR.from_head_major(buf, b, tokens, heads), qkv)
    out_hm = attn(capi, buf, b, tokens, heads, d, pre=1, hm=1)
    out_rm = attn(capi, qkv, b, tokens, heads, d, pre=1, hm=0)
    assert torch.isfinite(out_hm).all() and torch.equal(out_hm, out_rm)


@pytest.mark.parametrize("dtype", DTYPES)
def test_qkv_projection_refuses_planes_at_576_tokens(capi, dtype):
    """24^2 = 576 tokens are not whole 256-row tiles: the projection reports 0 and writes rows"""
    heads, d, b, tokens = 8, 80, 16, 576
    m, n_out, k = b * tokens, 3 * heads * d, heads * d
    ops = _folded_projection(capi, dtype, m, n_out, k)
    rows, buf, wrote = _qkv_projections(capi, ops, dtype, m, n_out, k, heads, d, tokens)
    assert wrote == 0
    assert torch.isfinite(rows).all() and torch.equal(buf.reshape(m, n_out), rows)


# --------------------------------------------------------------------------------------------------------- f. the largest tensor the persistent kernel accepts
@pytest.mark.parametrize("dtype", DTYPES)
def test_self_attention_largest_admitted_tensor(capi, dtype):
    """The persistent kernel addresses the QKV tensor with 32-bit byte offsets under one buffer descriptor and is dispatched below 4 GiB: d = 40, N = 4096, 8 heads,
    b = 546 is 4,293,918,720 bytes (admitted), b = 547 is not (the two-block kernel).  Every offset of the admitted launch stays inside the tensor, so below 2^32: an
    item's Q / K / V base plus a tile plus a lane's chunk is the address of a byte of the tensor (tiles past an item's last are the next item's first four, or -- for a
    block's last item -- its own last four); the output side uses 64-bit pointers.  Rows 0-15, 265-280 (across the 2 GiB offset) and 530-545 of the big call equal
    16-row calls on those slices (items are independent) and meet the fp32 reference; everything is finite.  Both layouts."""
    heads, d, n = 8, 40, 4096
    b = 546
    assert 3 * b * n * heads * d * 2 == 4293918720
    assert AR.self_attention_route(b, n, heads, d, n_cu()) == "d40-persistent" and AR.self_attention_route(b + 1, n, heads, d, n_cu()) == "d40-two-block"
    assert AR.self_attention_route(16, n, heads, d, n_cu()) == "d40-persistent"
    g = torch.Generator(device="cuda").manual_seed(546)
    big = torch.empty(b + 1, n, 3 * heads * d, dtype=dtype, device="cuda")
    for r0 in range(0, b + 1, 64):
        big[r0:r0 + 64] = torch.randn(big[r0:r0 + 64].shape, generator=g, device="cuda").to(dtype)
    big = AR.prescale_q(big, heads, d)
    qkv = big[:b]                                         # (a contiguous prefix)
    groups = [0, 265, 530]
    assert 265 * n * 3 * heads * d * 2 < 1 << 31 < 281 * n * 3 * heads * d * 2
    refs = {r0: AR.ref_self_attention(qkv[r0:r0 + 16], heads, prescaled=True) for r0 in groups}
    for hm in (0, 1):
        lay = (lambda t: AR.to_head_major(t, heads)) if hm else (lambda t: t.contiguous())
        out = attn(capi, lay(qkv), b, n, heads, d, pre=1, hm=hm)
        assert torch.isfinite(out).all()
        for r0 in groups:
            part = attn(capi, lay(qkv[r0:r0 + 16]), 16, n, heads, d, pre=1, hm=hm)
            assert torch.equal(out[r0:r0 + 16], part), f"rows {r0}..{r0 + 15} of the {b}-row call differ from the 16-row call (head_major={hm})"
            AR.check_attention(out[r0:r0 + 16], refs[r0], heads, d, dtype, 1.0, f"largest_tensor rows={r0}.. head_major={hm} route=d40-persistent prescaled=1")
        del out
    out = attn(capi, big, b + 1, n, heads, d, pre=1)     # one row more: the two-block kernel, 64-bit addresses
    assert torch.isfinite(out).all()
    for r0 in groups:
        AR.check_attention(out[r0:r0 + 16], refs[r0], heads, d, dtype, 1.0, f"largest_tensor+1 rows={r0}.. route=d40-two-block prescaled=1")
    last = AR.ref_self_attention(big[b:], heads, prescaled=True)
    AR.check_attention(out[b:], last, heads, d, dtype, 1.0, "largest_tensor+1 last row route=d40-two-block prescaled=1")


# --------------------------------------------------------------------------------------------------------- g. cross-attention on rows [u_t, c_s, c_t]
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d", [(256, 160), (1024, 80), (4096, 40)])
def test_cross_attention_three_row_call_equals_rows_of_the_four_row_call(capi, dtype, n, d):
    """ctrl.first_row = n_img: the call carries rows [u_t, c_s, c_t] (the Refine + Reweight edit on c_t reads the keys of the c_s row in front of it, the map store
    takes c_s and c_t).  Both calls run the same two kernel instantiations (plain rows, edited rows), so outputs and stored maps equal those rows of the four-row
    call bit for bit."""
    from tests.test_kernels_gpu import _ptp_tables, rnd
    lib = capi.load()
    n_img, heads = 2, 8
    c = heads * d
    q4 = rnd(4 * n_img, n, c, seed=1, dtype=dtype)
    kv4 = rnd(4 * n_img, 77, 2 * c, seed=2, dtype=dtype)
    mapper, alphas, eq, ca = _ptp_tables(n_img)
    res = {}
    for first_row in (0, n_img):
        b = 4 * n_img - first_row
        q, kv = q4[first_row:].contiguous(), kv4[first_row:].contiguous()
        out = torch.full((b, n, c), SENTINEL, dtype=dtype, device="cuda")
        maps = torch.zeros(5, n_img, 2, heads, n, 77, dtype=torch.float32, device="cuda")
        ctrl = capi.AttnCtrl(mode=capi.ATTN_PTP, n_img=n_img, store_maps=1, mapper=capi.ptr(mapper), alphas=capi.ptr(alphas), equalizer=capi.ptr(eq),
                             cross_alpha=capi.ptr(ca), first_row=first_row)
        for _ in range(2):
            capi.check(lib.etainv_op_cross_attention(capi.ptr(q), capi.ptr(kv), capi.ptr(out), b, n, heads, d, 77, C.byref(ctrl), 3, n_img, capi.ptr(maps),
                                                     capi.dtype_code(dtype), capi.stream_ptr()))
        torch.cuda.synchronize()
        res[first_row] = (out, maps)
    out4, maps4 = res[0]
    out3, maps3 = res[n_img]
    assert torch.isfinite(out3).all() and float(maps3[3].abs().max()) > 0.0
    assert torch.equal(out3, out4[n_img:])
    assert torch.equal(maps3, maps4)
