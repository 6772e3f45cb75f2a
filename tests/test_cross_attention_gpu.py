"""Cross-attention (cross_attn_kernel, 16-bit; cross_attn_f32_kernel) through etainv_op_cross_attention, per element: every term of the prompt-to-prompt edit
(Refine / Replace, Reweight, time blend with fractional weights), both first rows of layout 2, layouts 1 and 3, the map store per element with exact zeros
outside its slots, contexts shorter than 77 tokens, sharper softmaxes, ragged / multi-block / XCD-dealt launches, coded inputs that name the rows, tokens and
table entries an output was computed from, refusals that launch nothing, and run-to-run identity.
References, emulation, inputs and the list of cases: tests/cross_attention_ref.py (checked on the CPU by tests/test_cross_attention_ref.py, including that the
emulation of the unavoidable loss uses at most half of every bound on exactly these inputs).  ETAINV_ATTN_MARGINS=1 with pytest -s prints the emulation's
figures beside the kernel's (profiles/cross_attention_parity_margins.log is such a run)."""
import ctypes as C

import pytest
import torch

from tests import cross_attention_ref as XR

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16, torch.float32]
HEADS = XR.HEADS
SENTINEL = 7.0
GUARD = 4096        # elements appended to the output and put around the map store


@pytest.fixture(scope="module")
def capi():
    from etainv import _capi
    _capi.load()
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _capi


def launch(capi, q, kv, d, dtype, n_ctx=XR.CTX, mode=None, n_img=1, first_row=0, src_exit_block=0, tables=None, store=True, n_layers=XR.N_LAYERS, map_layer=XR.MAP_LAYER,
           n_img_cap=1, calls=1, maps_fill=0.0, with_maps=True, rows=None):
    """-> (status of the last call, out [b][N][C], out's guard, maps [n_layers][n_img_cap][2][heads][N][77], the maps' two guards); nothing is asserted here"""
    lib = capi.load()
    b, n, c = q.shape
    rows = b if rows is None else rows          # (a refusal test passes a row count of its own; the tensors keep their size)
    qd, kvd = q.cuda().contiguous(), kv.cuda().contiguous()
    out_all = torch.full((b * n * c + GUARD,), SENTINEL, dtype=dtype, device="cuda")
    n_maps = n_layers * n_img_cap * 2 * HEADS * n * XR.CTX
    maps_all = torch.full((n_maps + 2 * GUARD,), maps_fill, dtype=torch.float32, device="cuda")
    maps = maps_all[GUARD:GUARD + n_maps]
    tabs = {k: (None if v is None else v.cuda().contiguous()) for k, v in (tables or {}).items()}
    ctrl = None
    if mode is not None:
        ctrl = capi.AttnCtrl(mode=mode, n_img=n_img, store_maps=int(store), first_row=first_row, src_exit_block=src_exit_block,
                             **{k: capi.ptr(v) for k, v in tabs.items()})
    st = 0
    for _ in range(calls):
        st = lib.etainv_op_cross_attention(capi.ptr(qd), capi.ptr(kvd), capi.ptr(out_all), rows, n, HEADS, d, n_ctx, C.byref(ctrl) if ctrl is not None else None,
                                           map_layer, n_img_cap, capi.ptr(maps) if with_maps else None, capi.dtype_code(dtype), capi.stream_ptr())
        if st != 0:
            break
    torch.cuda.synchronize()
    return (st, out_all[:b * n * c].reshape(b, n, c).cpu(), out_all[b * n * c:].cpu(), maps.reshape(n_layers, n_img_cap, 2, HEADS, n, XR.CTX).cpu(),
            torch.cat([maps_all[:GUARD], maps_all[GUARD + n_maps:]]).cpu())


def run_case(capi, case):
    """the launch of a Case (tests/cross_attention_ref.py): layout 2 = prompt-to-prompt, 3 = the same behind src_exit_block, 1 = store mode"""
    mode = capi.ATTN_STORE if case.layout == 1 else capi.ATTN_PTP
    st, out, out_guard, maps, maps_guard = launch(capi, case.q, case.kv, case.d, case.dtype, n_ctx=case.n_ctx, mode=mode, n_img=case.n_img, first_row=case.first_row,
                                                  src_exit_block=12 if case.layout == 3 else 0, tables=case.tables, n_img_cap=case.n_img_cap, calls=XR.CALLS)
    capi.check(st)
    return out, out_guard, maps, maps_guard


def check_case(case, out, out_guard, maps, maps_guard):
    """the output at all three grains against float64; the stored maps per element against 2 x float64 within MAP_MARGIN x the emulation's own worst error (a bound
    from the reference side only), below the old global ceiling of 1e-3; everything outside the stored slots exactly 0; the guards intact"""
    assert torch.isfinite(out).all() and bool((out_guard == SENTINEL).all()), (case.label, "output guard overwritten")
    XR.check_attention(out, case.ref, HEADS, case.d, case.dtype, 1.0, "cross " + case.label, emulate=lambda: case.emu)
    ref = XR.ref_maps(case.ref_probs, *case.map_args())
    mask = XR.stored_mask(case.ref_probs, *case.map_args())
    assert float(maps_guard.abs().max()) == 0.0, (case.label, "a store outside the map tensor")
    stray = torch.nonzero((maps != 0) & ~mask)
    assert len(stray) == 0, (case.label, "stored outside the slots, first at (layer, image, role, head, query, token)", stray[0].tolist(), len(stray))
    err = (maps.double() - ref).abs()
    worst, emu = float(err.max()), case.emulation_map_error()
    bound = XR.MAP_MARGIN * emu
    rel = float((maps.double() - ref).norm() / ref.norm())
    print(f"cross-map-parity {case.label} dtype={str(case.dtype).split('.')[-1]} kernel: max|maps - {XR.CALLS} ref|={worst:.3e} global={rel:.3e} "
          f"emulation: max|p - ref|={emu:.3e} ratio={worst / emu if emu else 0.0:.2f} bound: {bound:.3e}")
    assert worst <= bound, (case.label, "map element (layer, image, role, head, query, token)", torch.nonzero(err == err.max())[0].tolist(), worst, bound)
    assert rel < 1e-3
    return worst, emu


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,n_img,fr,kind,gain", XR.EDIT_CASES)
def test_cross_edit_every_term(capi, dtype, n, d, n_img, fr, kind, gain):
    """Layout 2 at both first rows, Refine and Replace with tables whose every term is fractional somewhere and 0 / 1 somewhere (XR.edit_tables: a different draw per
    image, two wrapped mapper entries), gain 1 and 2, two calls into layer 1 of a 3-layer store with a spare image.  The map bound is MAP_MARGIN = 8 times the
    emulation's own worst error on one call's probabilities; measured on an MI355X (profiles/cross_attention_parity_margins.log, every case of this file): the kernel's
    error on the two-call sum is at most 2.84 times that (an ideal kernel: 2.0), worst at bf16, N = 200, d = 160, Replace, gain 1."""
    case = XR.edit_case(dtype, n, d, n_img, fr, kind, gain)
    assert float((case.ref_probs[-n_img:] - XR.ref_cross_attention(case.q, case.kv, HEADS, XR.CTX, 0, n_img, 0, None)[1][-n_img:]).abs().max()) > 1e-2   # the edit matters
    check_case(case, *run_case(capi, case))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_ctx,n,d,n_img,fr,kind,gain", XR.SHORT_CASES)
def test_cross_short_context(capi, dtype, n_ctx, n, d, n_img, fr, kind, gain):
    """n_ctx < 77: kv rows of stride n_ctx, a key mask, mapper entries that wrap by n_ctx, tables and maps of stride 77 whose entries past n_ctx are NaN / stay 0."""
    case = XR.edit_case(dtype, n, d, n_img, fr, kind, gain, n_ctx=n_ctx)
    assert case.kv.shape == (case.b, n_ctx, 2 * HEADS * d) and case.kv.is_contiguous()
    out, out_guard, maps, maps_guard = run_case(capi, case)
    check_case(case, out, out_guard, maps, maps_guard)
    assert float(maps[..., n_ctx:].abs().max()) == 0.0
    if n_ctx == 1:
        # every probability is 1 before the edit: an unedited row is V of token 0 as it is, an edited one V of token 0 times the edited weight
        v0 = case.kv[:, 0, HEADS * d:]
        assert torch.equal(out[:-n_img], v0[:-n_img, None, :].expand(-1, n, -1))
        w = case.ref_probs[-n_img:, :, :, 0]                                               # [n_img][heads][N]
        assert float((w - w[:, :, :1]).abs().max()) == 0.0 and float((w - 1).abs().min()) > 1e-3
        want = v0[-n_img:].double().reshape(n_img, 1, HEADS, d) * w.permute(0, 2, 1)[..., None]
        assert float((case.ref[-n_img:] - want.reshape(n_img, n, -1)).abs().max()) < 1e-12


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout,rows,n,d,n_img", XR.STORE_CASES)
def test_cross_store_layouts(capi, dtype, layout, rows, n, d, n_img):
    """Layout 1 (store mode) with n_img and 2 n_img rows; layout 3 (prompt-to-prompt behind ctrl.src_exit_block: rows [u_t, c_t, c_s], later [u_t, c_t]) with edit
    tables that it must ignore: the outputs equal the plain reference and c_t / c_s land in role slots 1 / 0."""
    case = XR.store_case(dtype, layout, rows, n, d, n_img)
    assert (case.tables is not None) == (layout == 3)
    out, out_guard, maps, maps_guard = run_case(capi, case)
    check_case(case, out, out_guard, maps, maps_guard)
    stored = maps[XR.MAP_LAYER, :n_img].abs().amax(dim=(0, 2, 3, 4))                       # per role slot
    assert float(stored[0]) > 0 or rows == 2 and layout == 3
    assert (float(stored[1]) > 0) == (layout == 3)
    if layout == 3 and rows == 2:
        assert float(stored[0]) == 0.0                                                     # the source rows have left


def _first_wrong_slot(maps, slots, n_img_cap):
    for (img, slot), want in sorted(slots.items()):
        got = maps[XR.MAP_LAYER, img, slot].argmax(-1)                                     # [heads][N]
        bad = torch.nonzero(got != want[:, None])
        if len(bad):
            h, qy = bad[0].tolist()
            return f"map slot (image {img}, role {slot}): head {h} query {qy} has its maximum at token {int(got[h, qy])}, expected {int(want[h])}"
    return None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [40, 160])
@pytest.mark.parametrize("layout,fr,rows", [(2, 0, 4), (2, 1, 3), (1, 0, 2), (3, 1, 3)])
def test_cross_coded_roles_and_tables(capi, dtype, d, layout, fr, rows):
    """Coded inputs (XR.coded_roles, XR.coded_tables): integer equalities on ids decoded from output signs and stored maps.  (a) the softmax of (queries of row rq,
    keys of row rk, head h) is a 30-nat peak at a token that names the pair, V carries token and row: with the identity Refine a c_t row of layout 2 must name
    (Q, K of its c_s row; V of itself), every other row itself, and each stored slot the row it was filled from.  (b) layout 2: replace_mat of image i sends all mass
    to token 10 + i with equalizer 1 + i / 4 there: c_t of image i names that token and its slot holds that value in that column, 0 elsewhere."""
    n, n_img = 200, 4
    b = rows * n_img
    mode = capi.ATTN_STORE if layout == 1 else capi.ATTN_PTP
    kw = dict(mode=mode, n_img=n_img, first_row=fr * n_img, src_exit_block=12 if layout == 3 else 0, n_img_cap=n_img)
    # (a)
    q, kv = XR.coded_roles(b, n, HEADS, d, dtype)
    st, out, _, maps, _ = launch(capi, q, kv, d, dtype, tables=None if layout == 1 else XR.identity_refine(n_img), **kw)
    capi.check(st)
    tok, row, slots = XR.expected_roles(layout, n_img, fr * n_img, b, HEADS, edit=True)
    got_tok, got_row = XR.decode(out, HEADS, d)
    assert (msg := XR.first_mismatch(got_tok, tok[:, None, :], "Q / K rows (token of the peak)")) is None, msg
    assert (msg := XR.first_mismatch(got_row, row[:, None, None], "V row")) is None, msg
    assert (msg := _first_wrong_slot(maps, slots, n_img)) is None, msg
    assert len(slots) == int((maps[XR.MAP_LAYER].abs().amax(dim=(2, 3, 4)) > 0).sum()) and float(maps[XR.MAP_LAYER + 1].abs().max()) == 0.0
    if layout != 2:
        return
    # (b)
    q, kv = XR.coded_tables_q_kv(b, n, HEADS, d, dtype, 4)
    st, out, _, maps, _ = launch(capi, q, kv, d, dtype, tables=XR.coded_tables(n_img), **kw)
    capi.check(st)
    got_tok, got_row = XR.decode(out, HEADS, d)
    want_tok = XR.TABLE_TOKEN0 + torch.arange(n_img)
    assert (msg := XR.first_mismatch(got_tok[b - n_img:], want_tok[:, None, None], "token of the replace matrix (rows counted from the first c_t row)")) is None, msg
    assert (msg := XR.first_mismatch(got_row, row[:, None, None], "V row")) is None, msg
    slot = maps[XR.MAP_LAYER, :, 1]                                                        # [image][heads][N][77]
    ids = torch.stack([((slot[i, :, :, XR.TABLE_TOKEN0 + i] - 1) * 4).round().long() for i in range(n_img)])      # equalizer id: (1 + i / 4 - 1) * 4 = i
    assert (msg := XR.first_mismatch(ids.permute(0, 2, 1), torch.arange(n_img)[:, None, None], "equalizer entry in the stored map (rows = images)")) is None, msg
    col = torch.stack([slot[i, :, :, XR.TABLE_TOKEN0 + i] for i in range(n_img)])
    assert float((col - (1 + torch.arange(n_img)[:, None, None] / 4)).abs().max()) < 1e-5   # the value itself: the source row sums to 1 within fp32 rounding
    for i in range(n_img):
        slot[i, :, :, XR.TABLE_TOKEN0 + i] = 0
    assert float(slot.abs().max()) == 0.0, "mass outside the replace matrix's column"


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_refusals_launch_nothing(capi, dtype):
    """Every call of XR.REFUSALS returns non-zero with its message in etainv_last_error and leaves a sentinel-filled output and map store untouched.  (The tensors
    are those of the largest call of the list.)"""
    lib = capi.load()
    n = 40
    for name, over, fragment in XR.REFUSALS:
        a = dict(XR.REFUSAL_BASE, **over)
        d = a["d"]
        q, kv = XR.random_q_kv(8, n, HEADS, d, XR.CTX + 1, dtype, 0)
        tables = dict(XR.edit_tables(max(a["n_img"], 1), XR.CTX, 0))
        if not a["mapper"]:
            tables["mapper"] = tables["alphas"] = None
        if not a["cross_alpha"]:
            tables["cross_alpha"] = None
        st, out, out_guard, maps, maps_guard = launch(capi, q, kv, d, dtype, rows=a["b"], n_ctx=a["n_ctx"], mode=capi.ATTN_PTP if a["mode"] == "ptp" else capi.ATTN_STORE,
                                                      n_img=a["n_img"], first_row=a["first_row"], src_exit_block=a["src_exit_block"], tables=tables, store=bool(a["store"]),
                                                      n_img_cap=a["n_img_cap"], maps_fill=SENTINEL, with_maps=a["maps"])
        err = lib.etainv_last_error()
        assert st != 0 and fragment.encode() in err, (name, st, err)
        assert bool((out == SENTINEL).all()) and bool((out_guard == SENTINEL).all()) and bool((maps == SENTINEL).all()) and bool((maps_guard == SENTINEL).all()), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_two_runs_bit_identical(capi, dtype):
    """one edit + store call (N = 360: two blocks per (row, head), ragged, XCD-dealt) twice: equal bits in the outputs and in the maps"""
    case = XR.edit_case(dtype, *XR.EDIT_CASES[9])
    assert case.n == 360 and case.n_img == 4
    a, b = run_case(capi, case), run_case(capi, case)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and float(a[2].abs().max()) > 0
