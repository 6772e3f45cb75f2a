"""Every route of launch_igemm (csrc/igemm.hip: the rings, the two-slot kernels with and without split-K; csrc/ppgemm.hip; csrc/ppconv.hip; the fp32 twin of
csrc/f32path.hip) per element against float64, through the C ABI, at the smallest shapes that meet the routes' tile-count thresholds.

Each case of tests/gemm_ref.py runs in two input families: `random` against a counted bound, `exact` (small hashed integers) bit for bit.  After the one launch
the test asserts, in this order: the plan the library reports for it (etainv_op_last_igemm_plan: route, tile, K split, ppconv form / dual-N kind) -- a test
written for one kernel cannot silently test another after a threshold moves --, the guards behind the NaN-filled outputs and statistics buffers, the per-element
bound or the equality, the producer partials, and the reported stat_P / wm.  Every operand sits exactly sized between NaN margins (with_tail), so that a read
past either end reaches the output.  References, bounds, inputs and the case list: tests/gemm_ref.py, checked on the CPU by tests/test_gemm_ref.py.
`pytest -s` prints the worst error / bound ratio per case (profiles/gemm_parity_margins.log is such a run)."""
import ctypes as C
import os

import pytest
import torch

from tests import gemm_ref as G
from tests.test_aux_kernels_gpu import MARK, assert_guard, guarded, guarded_flat, last_plan
from tests.test_kernels_gpu import capi  # noqa: F401  (fixture)
from tests.test_norm_gpu import NAN, assert_tail, nan_buffer, offender, with_tail

pytestmark = pytest.mark.gpu

_ORDER = {c.name: i for i, c in enumerate(G.CASES)}
_FIRST = {}
for _c in G.CASES:
    _FIRST.setdefault(_c.shape_key, _ORDER[_c.name])
# the epilogue variants of one shape next to each other per (dtype, family): they share the operands on the device and the float64 products
PARAMS = sorted(G.PARAMS, key=lambda p: (_FIRST[G.CASE[p[0]].shape_key], G.NAME[p[1]], p[2], _ORDER[p[0]]))
_shared = {}


def shared_operands(case, dtype, family):
    key = (case.shape_key, dtype, family)
    if _shared.get("key") != key:
        _shared.clear()
        torch.cuda.empty_cache()
        o = G.case_operands(case, dtype, family)
        dev = {k: with_tail(v).reshape(v.shape) for k, v in vars(o).items() if torch.is_tensor(v) and k not in ("a1", "a2")}
        _shared.update(key=key, dev=dev)
    o = G.types.SimpleNamespace(**_shared["dev"])
    # the two sources are separate allocations, each with its own margins
    if "a1" not in _shared:
        _shared["a1"] = with_tail(o.a[:, : case.k1].contiguous()).reshape(-1, case.k1)
        _shared["a2"] = with_tail(o.a[:, case.k1:].contiguous()).reshape(-1, case.k2) if case.k2 else None
    o.a1, o.a2 = _shared["a1"], _shared["a2"]
    if "prod" not in _shared:
        _shared["prod"] = G.accumulate(case, o.a1, o.a2, o.w, torch.float64)
    return o, _shared["prod"]


def test_premises():
    # the thresholds are read once per process: the plans of the case list are those of the defaults
    for name in ("ETAINV_RING_MIN_TILES", "ETAINV_PPCONV_MIN_TILES", "ETAINV_DUALN_MIN_TILES", "ETAINV_DEEPK_MIN_TILES", "ETAINV_DEEPK_MIN_NK", "ETAINV_SPLITK_MAX",
                 "ETAINV_GEGLU_RING_MINK", "ETAINV_NO_RING", "ETAINV_NO_SPLITK", "ETAINV_DUALN", "ETAINV_PPCONV", "ETAINV_PPCONV2", "ETAINV_PATCHCONV", "ETAINV_UPS4"):
        assert name not in os.environ, name


def launch(capi, case, o, dtype, out, part, reported):
    """the case's one launch -> the status"""
    lib, p, dt, st = capi.load(), capi.ptr, capi.dtype_code(dtype), capi.stream_ptr()
    c = case
    bias = p(o.bias) if (c.bias or c.ln) else None
    res = p(o.res_used) if c.res else None
    k = c.k1 + c.k2
    if c.entry == "gemm":
        return lib.etainv_op_gemm(p(o.a1), p(o.w), bias, res, p(out), c.m, c.n, k, int(c.geglu), dt, st)
    if c.entry == "gemm_f32out":
        return lib.etainv_op_gemm_f32out(p(o.a1), p(o.w), bias, p(out), c.m, c.n, k, dt, st)
    if c.entry == "gemm_ln":
        if c.ln:
            return lib.etainv_op_gemm_ln(p(o.a1), p(o.w), bias, p(o.s), p(o.stat), None, p(out), None, None, c.m, c.n, k, int(c.geglu), dt, st)
        return lib.etainv_op_gemm_ln(p(o.a1), p(o.w), bias, None, None, res, p(out), p(part), C.byref(reported), c.m, c.n, k, 0, dt, st)
    if c.entry == "gemm_gn":
        return lib.etainv_op_gemm_gnstat(p(o.a1), p(o.w), bias, res, p(out), p(part), C.byref(reported), c.m, c.n, k, c.rows_per_image, dt, st)
    if c.entry == "gemm_hm":
        return lib.etainv_op_gemm_ln_hm(p(o.a1), p(o.w), bias, p(o.s), p(o.stat), p(out), c.m, c.n, k, 8, c.n // 24, c.hm, C.byref(reported), dt, st)
    if c.entry == "per_image":
        return lib.etainv_op_gemm_per_image(p(o.a1), p(o.w), bias, res, p(out), c.images, c.rows_per_image, c.n, k, dt, st)
    h, w = (c.h, c.w) if c.kind == "conv" else (1, c.rows_per_image)
    if c.entry == "conv_ex":
        return lib.etainv_op_conv3x3_ex(p(o.a1), p(o.w), bias, res, p(out), c.images, h, w, c.k1, c.n, c.stride, c.ups, c.pad0, 0, 0, dt, st)
    if c.entry == "conv_gn":
        return lib.etainv_op_conv3x3_gnstat(p(o.a1), p(o.w), bias, p(o.time), res, p(out), p(part), C.byref(reported), c.images, h, w, c.k1, c.n, dt, st)
    assert c.entry == "conv"
    time, stride = (o.time_ptr, o.time_stride) if c.time else (None, c.n)
    return lib.etainv_op_conv3x3_rv(p(o.a1), p(o.a2), c.k1, c.k2, p(o.w), bias, time, stride, res, p(out), c.images, h, w, c.n, c.stride, c.ups, c.taps, dt, st)


def check(capi, case, dtype, family, expect=None, env_label=""):
    """one launch of the case and every assertion on it -> the stored rows [m][n_out]"""
    lib = capi.load()
    c = case
    o, prod = shared_operands(c, dtype, family)
    label = f"{c.name}{env_label} {G.NAME[dtype]} {family}"
    out_t = torch.float32 if c.f32out else dtype
    if c.res:
        o.res_used = o.res if c.n_out == c.n else with_tail(o.res[:, : c.n_out].contiguous())
    if c.time:
        if c.time_strided:
            # the layer's columns inside the NaN-filled matrix of all time projections
            mat = torch.full((c.images, G.TIME_COLUMNS), NAN, dtype=torch.float32, device="cuda")
            mat[:, G.TIME_OFFSET:G.TIME_OFFSET + c.n] = o.time
            o.time_keep, o.time_ptr, o.time_stride = mat, mat.data_ptr() + 4 * G.TIME_OFFSET, G.TIME_COLUMNS
        else:
            o.time_ptr, o.time_stride = o.time.data_ptr(), c.n
    if c.ups == 2:
        # the phase weights as etainv_op_pack_ups4 leaves them: the fp32 sums of the taps that share a source pixel, rounded once -- bit for bit
        w4 = guarded_flat(o.w.numel(), dtype, 4096)
        capi.check(lib.etainv_op_pack_ups4(capi.ptr(o.w32), capi.ptr(w4), c.n, c.k1, capi.dtype_code(dtype), capi.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(w4[: o.w.numel()], o.w.flatten()) and bool((w4[o.w.numel():] == MARK).all()), f"{label}: etainv_op_pack_ups4"
    n_part = c.m * (c.n // G.LN_CHUNK) * 2 if c.lnprod else (c.m // G.GN_ROWS) * 2 * c.n if c.gnprod else 0
    part = nan_buffer(n_part) if n_part else None
    reported = C.c_int(-1)
    out = guarded(c.m, c.n_out, out_t)
    capi.check(launch(capi, c, o, dtype, out, part, reported))
    # 1. the plan
    want = expect or c.plan_for(dtype)
    plan = last_plan(capi)
    assert plan == want, f"{label}: launch_igemm took {plan}, the case is written for {want}"
    # 2. guards and tails
    assert_guard(out, c.m)
    if n_part:
        assert_tail(part, n_part, "partials")
    got = out[: c.m]
    if c.hm:
        assert reported.value == 1, f"{label}: the launch wrote row-major"
        got = got.flatten()[G.hm_index(c.m, c.n, 8, c.n // 24, c.hm, device="cuda")]
    # 3. per element
    ref, bound, _ = G.reference(c, o, dtype, plan["ksplit"], prod=prod)
    if family == "exact":
        same = got.double() == ref
        print(f"margin {label}: bit-equal {bool(same.all())}")
        assert bool(same.all()), f"{label}: {offender(got, ref, torch.full_like(ref, 1e-300))}"
    else:
        ratio = G.worst(got, ref, bound)
        print(f"margin {label}: kernel {ratio:.3f}")
        assert ratio <= 1.0, f"{label}: {offender(got, ref, bound)}"
    # 4. the partials, against statistics of the STORED rows; 5. what the launch reported
    if c.lnprod:
        pk = part[:n_part].reshape(c.m, -1, 2).double()
        want_p, (dm, dq) = G.ln_partials64(got), G.ln_partial_err(got)
        rm, rq = (pk[..., 0] - want_p[..., 0]).abs() / (dm + 1e-300), (pk[..., 1] - want_p[..., 1]).abs() / (dq + 1e-300)
        print(f"margin {label} LayerNorm partials: mean {float(rm.max()):.3f} M2 {float(rq.max()):.3f}")
        assert float(rm.max()) <= 1.0, f"{label}: partial mean, {offender(pk[..., 0], want_p[..., 0], dm + 1e-300)}"
        assert float(rq.max()) <= 1.0, f"{label}: partial M2, {offender(pk[..., 1], want_p[..., 1], dq + 1e-300)}"
    if c.gnprod:
        pk = part[:n_part].reshape(c.m // G.GN_ROWS, 2, c.n).double()
        rows = got[G.patch_rows(c.images, c.h, c.w, device="cuda")] if plan["route"] in ("ppconv", "ring-patch") else got
        want_p, err = G.gn_partials64(rows), G.gn_partial_err(rows)
        if family == "exact":
            assert torch.equal(pk, want_p), f"{label}: GroupNorm partials, {offender(pk, want_p, torch.full_like(want_p, 1e-300))}"
        else:
            rp = float(((pk - want_p).abs() / (err + 1e-300)).max())
            print(f"margin {label} GroupNorm partials: {rp:.3f}")
            assert rp <= 1.0, f"{label}: GroupNorm partials, {offender(pk, want_p, err + 1e-300)}"
    if c.lnprod or c.gnprod:
        assert reported.value == G.stat_report(c), f"{label}: reported {reported.value}"
    return got


@pytest.fixture(scope="module", autouse=True)
def release_shared():
    yield
    _shared.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("param", PARAMS, ids=G.param_id)
def test_route(capi, param):
    """Measured on an MI355X: profiles/gemm_parity_margins.log"""
    name, dtype, family = param
    check(capi, G.CASE[name], dtype, family)


@pytest.mark.parametrize("dtype", G.DTYPES16, ids=G.NAME.get)
def test_three_forms_of_one_conv(capi, dtype, monkeypatch):
    """13 x 32 x 32, 64 -> 1280 under the per-launch switches: the dual-M ping-pong kernel, its 256-pixel form and the ring's patch kernel, each held to the
    float64 bound on its own; the 256-pixel form and the patch kernel run the same K order and epilogue arithmetic and must agree bit for bit"""
    case = G.CASE["ppconv-dualm-gnprod"]
    check(capi, case, dtype, "random")
    monkeypatch.setenv("ETAINV_PPCONV2", "0")
    one = check(capi, case, dtype, "random", dict(route="ppconv", bm=256, bn=160, ksplit=1, form=0), " (256-pixel form)").clone()
    monkeypatch.setenv("ETAINV_PPCONV", "0")
    patch = check(capi, case, dtype, "random", dict(route="ring-patch", bm=256, bn=160, ksplit=1, form=0), " (ring-patch)")
    assert torch.equal(one, patch)


def test_refusals(capi):
    """what the launchers decline, each by its message, with nothing launched"""
    lib, p, st, dt = capi.load(), capi.ptr, capi.stream_ptr(), capi.F16
    z = lambda *s: torch.zeros(*s, dtype=torch.float16, device="cuda")  # noqa: E731
    f = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")  # noqa: E731
    out = torch.full((4096 * 1280,), MARK, dtype=torch.float16, device="cuda")
    x, w, bias = z(4096, 128), z(1280 * 9, 128), f(1280)
    refused = [
        # a phase form below the ring's threshold (1 x 16 x 16 -> 1024 rows: 32 tiles)
        ("phase form", lambda: lib.etainv_op_conv3x3_rv(p(x), None, 64, 0, p(w), p(bias), None, 1280, None, p(out), 1, 16, 16, 1280, 1, 2, 4, dt, st)),
        # per-image weights with an M tile that spans two images
        ("per-image weights", lambda: lib.etainv_op_gemm_per_image(p(x), p(w), p(f(2, 320)), None, p(out), 2, 100, 320, 128, dt, st)),
        ("rowvec_stride", lambda: lib.etainv_op_conv3x3_rv(p(x), None, 64, 0, p(w), p(bias), p(f(2, 1280)), 1276, None, p(out), 2, 16, 16, 1280, 1, 0, 9, dt, st)),
        ("GEGLU needs", lambda: lib.etainv_op_gemm(p(x), p(w), p(bias), None, p(out), 256, 192, 128, 1, dt, st)),
        ("folded LayerNorm: no residual", lambda: lib.etainv_op_gemm_ln(p(x), p(w), p(bias), p(f(320)), p(f(256, 2)), p(z(256, 320)), p(out), None, None, 256, 320,
                                                                        128, 0, dt, st)),
    ]
    for message, call in refused:
        assert call() != 0, message
        assert message in lib.etainv_last_error().decode(), (message, lib.etainv_last_error().decode())
        if message != "rowvec_stride":                       # (refused by the entry point, in front of launch_igemm)
            assert last_plan(capi)["route"] is None, "a refused launch leaves no plan"
    torch.cuda.synchronize()
    assert bool((out == MARK).all()), "a refused call launches nothing"
    # hm_* on a launch igemm_hm_ok declines (the ring is not filled): etainv_op_gemm_ln_hm asks first and launches the row-major form
    wrote = C.c_int(-1)
    capi.check(lib.etainv_op_gemm_ln_hm(p(x), p(w), p(f(960)), p(f(960)), p(f(512, 2)), p(out), 512, 960, 128, 8, 40, 256, C.byref(wrote), dt, st))
    assert wrote.value == 0 and last_plan(capi)["route"] == "two-slot"
    torch.cuda.synchronize()
    assert bool((out[512 * 960:] == MARK).all())
