"""GroupNorm, LayerNorm and their statistics chains (csrc/norm.hip, the fp32 twins of csrc/f32path.hip) per element and per (image, group) / per row, through the C
ABI: etainv_op_groupnorm at every stats / apply instantiation and launch-geometry branch, etainv_op_groupnorm_pre on hand-made producer partials (final_stats, the
scale / shift planes and the output), etainv_op_layernorm, etainv_op_row_stats, etainv_op_ln_finalize on hand-made (mean, M2) partials, the folded-LayerNorm consumer
of etainv_op_gemm_ln on off-centre rows, and the launchers' refusals.
References, emulation, bounds (counted roundings, no tuned constant), inputs and the case lists: tests/norm_ref.py, checked on the CPU by tests/test_norm_ref.py --
including that the emulation uses at most half of every bound on exactly these inputs.  Every output is NaN-filled with a guard region behind it; every input,
partial and scratch buffer is exactly sized with NaN around it, so that a read past either end reaches the output.  `pytest -s` prints, per case, the worst ratio of
error to bound of the kernel and of the emulation (profiles/norm_parity_margins.log is such a run)."""
import os

import pytest
import torch

from tests import norm_ref as NR
from tests.test_aux_kernels_gpu import MARK, U_RND, assert_guard, guarded
from tests.test_kernels_gpu import capi  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

MARGIN = 16384       # NaN elements in front of and behind every input, partial and scratch buffer
NAN = float("nan")
IDS = NR.NAME.get


def with_tail(t):
    """the tensor's values on the device, exactly sized, NaN in front of them and behind them"""
    t = t.contiguous().flatten().cuda()
    pad = torch.full((MARGIN,), NAN, dtype=t.dtype, device="cuda")
    return torch.cat([pad, t, pad])[MARGIN:MARGIN + t.numel()]


def nan_buffer(n):
    """n floats the kernel must write before it reads them, NaN behind them"""
    return torch.full((n + MARGIN,), NAN, dtype=torch.float32, device="cuda")


def assert_tail(buf, n, what):
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[n:]).all()), f"{what}: written behind its {n} elements"
    assert bool(torch.isfinite(buf[:n]).all()), f"{what}: an element left unwritten or not finite"


def offender(got, ref, bound):
    r = (got.double() - ref).abs() / bound
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    i = int(r.argmax())
    at = [int(v) for v in torch.unravel_index(torch.tensor(i), r.shape)]
    return f"worst at {at}: got {float(got.flatten()[i])!r}, reference {float(ref.flatten()[i])!r}, bound {float(bound.flatten()[i]):.3e} ({int((r > 1).sum())} of {r.numel()} outside)"


def assert_stats(label, mean_k, rstd_k, mean, rstd, dmean, drstd):
    """per (image, group) or per row"""
    em = (mean_k.double() - mean).abs() / (dmean + NR.U32 * mean.abs() + 1e-300)
    er = (rstd_k.double() - rstd).abs() / (rstd * drstd)
    print(f"margin {label} statistics: kernel mean {float(em.max()):.3f} rstd {float(er.max()):.3f}")
    assert float(em.max()) <= 1.0, f"{label}: mean, {offender(mean_k, mean, dmean + NR.U32 * mean.abs() + 1e-300)}"
    assert float(er.max()) <= 1.0, f"{label}: rstd, {offender(rstd_k, rstd, rstd * drstd)}"


def test_premises():
    assert NR.U_RND == U_RND
    # both are read once per process; the geometry premises of the cases are those of the defaults
    assert "ETAINV_GN_NOFLAT" not in os.environ and "ETAINV_GN_APPLY_BLOCKS" not in os.environ


# ---------------------------------------------------------------------------------------------------------------- a. GroupNorm, direct
@pytest.mark.parametrize("dtype", NR.DTYPES3, ids=IDS)
@pytest.mark.parametrize("name", [c[0] for c in NR.GN_CASES])
def test_groupnorm(capi, dtype, name):
    """SiLU with eps 1e-5 and no SiLU with eps 1e-6 on the same input.  16-bit types: the statistics from the per-chunk partial sums the stats kernel leaves in
    the scratch, against the conditioned bound; fp32: (mean, rstd) as the scratch holds them.
    Measured on an MI355X: profiles/norm_parity_margins.log"""
    lib = capi.load()
    case = NR.gn_case(dtype, name)
    b, hw, c1, c2, c, groups, geo = case.b, case.hw, case.c1, case.c2, case.c, case.groups, case.geo
    x, gamma, beta = case.x.cuda(), case.gamma.cuda(), case.beta.cuda()
    x1 = with_tail(x[..., :c1])
    x2 = with_tail(x[..., c1:]) if c2 else None
    n_scr = b * groups * 2 * (1 if dtype == torch.float32 else geo.chunks)
    for eps, silu in NR.EPS_SILU:
        out, scratch = guarded(b * hw, c, dtype), nan_buffer(n_scr)
        capi.check(lib.etainv_op_groupnorm(capi.ptr(x1), capi.ptr(x2), c1, c2, capi.ptr(gamma), capi.ptr(beta), capi.ptr(out), b, hw, groups, eps, silu,
                                           capi.ptr(scratch), capi.dtype_code(dtype), capi.stream_ptr()))
        assert_guard(out, b * hw)
        assert_tail(scratch, n_scr, "scratch")
        got = out[: b * hw].reshape(b, hw, c)
        r = case.evaluate(x, gamma, beta, eps, silu, got)
        print(f"margin {case.label} silu {silu}: kernel {r['kernel']:.3f} emulation {r['emulation']:.3f} (before its rounding {r['arithmetic']:.3f} of e"
              + (f", statistics in the kernel's order {r['kernel_order']:.3f}" if "kernel_order" in r else "") + ")")
        assert r["kernel"] <= 1.0, f"{case.label} silu {silu}: {offender(got, r['ref'], r['bound'])}"
        mean, _, rstd = NR.ref_gn_stats(x, groups, eps)
        if dtype == torch.float32:
            st = scratch[:n_scr].reshape(b, groups, 2)
            assert_stats(case.label, st[..., 0], st[..., 1], mean, rstd, *NR.stats_err_double(mean))
        else:
            sums = scratch[:n_scr].double().reshape(b, geo.chunks, groups, 2).sum(1)
            count = float(hw * geo.cpg)
            mean_k = sums[..., 0] / count
            rstd_k = ((sums[..., 1] / count - mean_k ** 2).clamp_min(0.0) + NR.f32(eps)).rsqrt()
            assert_stats(case.label, mean_k, rstd_k, mean, rstd, *NR.gn_stats_err16(x, groups, eps, geo))
        rstd0 = NR.f32(eps) ** -0.5
        if case.family == "const":
            # all sums exact, mean = 0.5 and var = 0 exact: beta itself (a multiple of 1/8) without SiLU
            if not silu:
                assert torch.equal(got.double(), beta.double()[None, None].expand(b, hw, c)), "a constant image normalises to beta"
            ref, bound, _ = NR.const_bound(0.5, rstd0, gamma, beta, silu, dtype)
            assert NR.worst(got, ref[None, None].expand(b, hw, c), bound[None, None].expand(b, hw, c) + 1e-300) <= 1.0
        if case.family == "group_const":
            g0 = NR.const_group(c, groups)
            sl = slice(g0 * geo.cpg, (g0 + 1) * geo.cpg)
            for i in range(b):
                ref, bound, _ = NR.const_bound(0.5 * float(NR.image_scales(b, case.family)[i]), rstd0, gamma[sl], beta[sl], silu, dtype)
                assert NR.worst(got[i, :, sl], ref[None].expand(hw, -1), bound[None].expand(hw, -1) + 1e-300) <= 1.0, f"{case.label}: the constant group of image {i}"


@pytest.mark.parametrize("dtype", NR.DTYPES16, ids=IDS)
def test_groupnorm_refuses_a_width_beyond_five_vectors_per_lane(capi, dtype):
    b, hw, c = 1, 8, 2816            # 352 channel vectors > 64 x 5; a multiple of 32 and of 8, so that only the width is at fault
    x = torch.zeros(b, hw, c, dtype=dtype, device="cuda")
    gamma, beta = torch.ones(c, device="cuda"), torch.zeros(c, device="cuda")
    out = torch.full((b * hw, c), MARK, dtype=dtype, device="cuda")
    scratch = torch.full((b * 65 * 64,), MARK, dtype=torch.float32, device="cuda")
    with pytest.raises(capi.EtainvError, match="C too large"):
        capi.check(capi.load().etainv_op_groupnorm(capi.ptr(x), None, c, 0, capi.ptr(gamma), capi.ptr(beta), capi.ptr(out), b, hw, 32, 1e-5, 1, capi.ptr(scratch),
                                                   capi.dtype_code(dtype), capi.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((out == MARK).all()) and bool((scratch == MARK).all()), "a refused call launches nothing"


# ---------------------------------------------------------------------------------------------------------------- b. GroupNorm from producer partials
def call_pre(capi, x1, x2, c1, c2, p1, wm1, p2, wm2, gamma, beta, out, b, hw, groups, eps, silu, final, dtype):
    return capi.load().etainv_op_groupnorm_pre(capi.ptr(x1), capi.ptr(x2), c1, c2, capi.ptr(p1), wm1, capi.ptr(p2), wm2, capi.ptr(gamma), capi.ptr(beta),
                                               capi.ptr(out), b, hw, groups, eps, silu, capi.ptr(final), capi.dtype_code(dtype), capi.stream_ptr())


@pytest.mark.parametrize("dtype", NR.DTYPES16, ids=IDS)
@pytest.mark.parametrize("family", NR.GN_PRE_FAMILIES)
@pytest.mark.parametrize("idx", range(len(NR.GN_PRE_CASES)))
def test_groupnorm_pre(capi, dtype, idx, family):
    """gn_finalize_kernel + the pre_scsh form of gn_apply_kernel.  The reference finalizes the same fp32 partials in float64: the sums are combined in double,
    so the centred bound applies whatever the offset"""
    case = NR.pre_case(dtype, idx, family)
    b, hw, c1, c2, c = case.b, case.hw, case.c1, case.c2, case.c
    x = torch.cat([case.x1] + ([case.x2] if c2 else []), -1).cuda()
    gamma, beta, p1c, p2c = case.gamma.cuda(), case.beta.cuda(), case.p1.cuda(), (case.p2.cuda() if c2 else None)
    x1, x2, p1, p2 = with_tail(case.x1), (with_tail(case.x2) if c2 else None), with_tail(case.p1), (with_tail(case.p2) if c2 else None)
    n_fin = b * (32 * 2 + 2 * c)
    for eps, silu in NR.EPS_SILU:
        out, final = guarded(b * hw, c, dtype), nan_buffer(n_fin)
        capi.check(call_pre(capi, x1, x2, c1, c2, p1, case.wm1, p2, case.wm2, gamma, beta, out, b, hw, 32, eps, silu, final, dtype))
        assert_guard(out, b * hw)
        assert_tail(final, n_fin, "final_stats")
        got = out[: b * hw].reshape(b, hw, c)
        r = case.evaluate(x, p1c, p2c, gamma, beta, eps, silu)
        st, planes = final[: b * 64].reshape(b, 32, 2), final[b * 64:n_fin].reshape(b, 2, c)
        assert_stats(case.label, st[..., 0], st[..., 1], r["mean"], r["rstd"], r["dmean"], r["drstd"])
        k_planes, k_out = NR.worst(planes, r["planes"], r["planes_bound"] + 1e-300), NR.worst(got, r["ref"], r["bound"])
        print(f"margin {case.label} silu {silu}: kernel {k_out:.3f} planes {k_planes:.3f} emulation {r['emulation']:.3f} (before its rounding {r['arithmetic']:.3f} of e)")
        assert k_planes <= 1.0, f"{case.label}: scale / shift planes, {offender(planes, r['planes'], r['planes_bound'] + 1e-300)}"
        assert k_out <= 1.0, f"{case.label} silu {silu}: {offender(got, r['ref'], r['bound'])}"
        if family == "const" and not silu:
            assert torch.equal(got.double(), beta.double()[None, None].expand(b, hw, c)), "a constant image normalises to beta"
            assert torch.equal(st[..., 0], torch.full_like(st[..., 0], 0.5))


@pytest.mark.parametrize("dtype", NR.DTYPES16, ids=IDS)
@pytest.mark.parametrize("what", ["hw % wm != 0", "groups = 64", "second source without its partials"])
def test_groupnorm_pre_refusals(capi, dtype, what):
    case = NR.pre_case(dtype, 1, "random")                    # (b = 2, hw = 256, 640 + 320, wm = 64 / 32)
    b, hw, c1, c2, c = case.b, case.hw, case.c1, case.c2, case.c
    x1, x2, p1, p2, gamma, beta = case.x1.cuda(), case.x2.cuda(), case.p1.cuda(), case.p2.cuda(), case.gamma.cuda(), case.beta.cuda()
    wm1, groups = case.wm1, 32
    if what == "hw % wm != 0":
        wm1 = 96
    elif what == "groups = 64":
        groups = 64
    else:
        p2 = None
    out = torch.full((b * hw, c), MARK, dtype=dtype, device="cuda")
    final = torch.full((b * (64 * 2 + 2 * c),), MARK, dtype=torch.float32, device="cuda")
    with pytest.raises(capi.EtainvError):
        capi.check(call_pre(capi, x1, x2, c1, c2, p1, wm1, p2, case.wm2, gamma, beta, out, b, hw, groups, 1e-5, 1, final, dtype))
    torch.cuda.synchronize()
    assert bool((out == MARK).all()) and bool((final == MARK).all()), "a refused call launches nothing"


# ---------------------------------------------------------------------------------------------------------------- c. LayerNorm and row statistics
LN_PARAMS = [(dt, c) for dt in NR.DTYPES3 for c in NR.LN_WIDTHS if dt != torch.float32 or c <= 1280]


@pytest.mark.parametrize("family", NR.LN_FAMILIES)
@pytest.mark.parametrize("dtype,c", LN_PARAMS, ids=[f"{NR.NAME[dt]}-{c}" for dt, c in LN_PARAMS])
def test_layernorm_and_row_stats(capi, dtype, c, family):
    """row counts 1, 3, 4, 5 (around the four rows of a block) and 130, each on a buffer of exactly that many rows"""
    lib = capi.load()
    x = NR.row_input(max(NR.LN_ROWS), c, dtype, family, seed=c).cuda()
    gamma, beta = (t.cuda() for t in NR.ln_params(c))
    eps = 1e-5
    ref, bound, e = NR.ln_bound(x, gamma, beta, eps, dtype)
    emu = NR.emulate_layernorm(x, gamma, beta, eps, dtype)
    mean, _, rstd = NR.ref_row_stats(x, eps)
    dmean, drstd = NR.row_stats_err(x, eps)
    for rows in NR.LN_ROWS:
        label = f"layernorm c={c} rows={rows} {family} {NR.NAME[dtype]}"
        xr, out = with_tail(x[:rows]), guarded(rows, c, dtype)
        capi.check(lib.etainv_op_layernorm(capi.ptr(xr), capi.ptr(gamma), capi.ptr(beta), capi.ptr(out), rows, c, eps, capi.dtype_code(dtype), capi.stream_ptr()))
        assert_guard(out, rows)
        got = out[:rows]
        k = NR.worst(got, ref[:rows], bound[:rows])
        print(f"margin {label}: kernel {k:.3f} emulation {NR.worst(emu[:rows].to(dtype), ref[:rows], bound[:rows]):.3f} "
              f"(before its rounding {NR.worst(emu[:rows], ref[:rows], e[:rows] + 1e-300):.3f} of e)")
        assert k <= 1.0, f"{label}: {offender(got, ref[:rows], bound[:rows])}"
        const = [r for r in NR.const_rows(rows)] if family == "const_row" else []
        if const:
            assert torch.equal(got[const], beta.to(dtype)[None].expand(len(const), c)), "a constant row normalises to beta exactly"
        if dtype != torch.float32:
            stat = nan_buffer(rows * 2)
            capi.check(lib.etainv_op_row_stats(capi.ptr(xr), capi.ptr(stat), rows, c, eps, capi.dtype_code(dtype), capi.stream_ptr()))
            assert_tail(stat, rows * 2, "row statistics")
            st = stat[: rows * 2].reshape(rows, 2)
            assert_stats("row_stats " + label, st[:, 0], st[:, 1], mean[:rows], rstd[:rows], dmean[:rows], drstd[:rows])
            if const:
                assert torch.equal(st[const, 0].double(), x[const, 0].double())


@pytest.mark.parametrize("dtype,c", [(torch.float16, 1544), (torch.bfloat16, 1544), (torch.float16, 324), (torch.bfloat16, 324), (torch.float32, 1288)],
                         ids=lambda v: NR.NAME.get(v, str(v)))
def test_layernorm_refusals(capi, dtype, c):
    lib = capi.load()
    rows = 5
    x = torch.zeros(rows, c, dtype=dtype, device="cuda")
    gamma, beta = torch.ones(c, device="cuda"), torch.zeros(c, device="cuda")
    out = torch.full((rows, c), MARK, dtype=dtype, device="cuda")
    stat = torch.full((rows, 2), MARK, dtype=torch.float32, device="cuda")
    with pytest.raises(capi.EtainvError):
        capi.check(lib.etainv_op_layernorm(capi.ptr(x), capi.ptr(gamma), capi.ptr(beta), capi.ptr(out), rows, c, 1e-5, capi.dtype_code(dtype), capi.stream_ptr()))
    if dtype != torch.float32:
        with pytest.raises(capi.EtainvError):
            capi.check(lib.etainv_op_row_stats(capi.ptr(x), capi.ptr(stat), rows, c, 1e-5, capi.dtype_code(dtype), capi.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((out == MARK).all()) and bool((stat == MARK).all()), "a refused call launches nothing"


# ---------------------------------------------------------------------------------------------------------------- d. etainv_op_ln_finalize
@pytest.mark.parametrize("cw", NR.LNF_CW)
@pytest.mark.parametrize("p", NR.LNF_P)
def test_ln_finalize(capi, p, cw):
    """hand-made (mean, M2) partials; the reference is the float64 merge of the same fp32 values, the bound that of the P sequential fp32 updates.  Row counts
    around the 256 rows of a block"""
    lib = capi.load()
    eps = 1e-5
    for family in NR.LNF_FAMILIES:
        part = NR.lnf_partials(max(NR.LNF_ROWS), p, cw, family, seed=p + cw).cuda()
        mean, rstd = NR.chan_merge(part, cw, eps)
        dmean, drstd = NR.ln_finalize_err(part, cw, eps)
        for rows in NR.LNF_ROWS:
            pr, stat = with_tail(part[:rows]), nan_buffer(rows * 2)
            capi.check(lib.etainv_op_ln_finalize(capi.ptr(pr), p, cw, eps, capi.ptr(stat), rows, capi.stream_ptr()))
            assert_tail(stat, rows * 2, "row statistics")
            st = stat[: rows * 2].reshape(rows, 2)
            assert_stats(f"ln_finalize P={p} cw={cw} rows={rows} {family}", st[:, 0], st[:, 1], mean[:rows], rstd[:rows], dmean[:rows], drstd[:rows])


# ---------------------------------------------------------------------------------------------------------------- e. the folded-LayerNorm consumer
@pytest.mark.parametrize("dtype", NR.DTYPES16, ids=IDS)
@pytest.mark.parametrize("m,c,n", NR.GEMM_LN_CASES)
def test_gemm_ln_on_off_centre_rows(capi, dtype, m, c, n):
    """rows at |mean| / std = 8: rstd (acc - mean s[n]) + c[n] subtracts two numbers eight times the result.  Statistics from etainv_op_row_stats, weights from
    etainv_op_ln_fold; against float64 LayerNorm(x) W'^T + c on those folded weights, one output rounding plus K 2^-24 rstd sum |x| |W'|"""
    lib = capi.load()
    dt, eps = capi.dtype_code(dtype), 1e-5
    x, w, gamma, beta, bias = (t.cuda() for t in NR.gemm_ln_inputs(m, c, n, dtype))
    wp = torch.full((n, c), NAN, dtype=dtype, device="cuda")
    s_vec, c_vec = nan_buffer(n), nan_buffer(n)
    capi.check(lib.etainv_op_ln_fold(capi.ptr(w), capi.ptr(gamma), capi.ptr(beta), capi.ptr(bias), n, c, 0, 1.0, capi.ptr(wp), capi.ptr(s_vec), capi.ptr(c_vec),
                                     dt, capi.stream_ptr()))
    assert_tail(s_vec, n, "s_vec")
    assert_tail(c_vec, n, "c_vec")
    s_vec, c_vec = s_vec[:n], c_vec[:n]
    # the fold: W' = W gamma rounded once, s its row sums, c = W beta + bias, each an fp32 sum of c terms
    wp_ref, s_ref, c_ref = NR.fold_ref(w, gamma, beta, bias, dtype)
    assert float(((wp.double() - wp_ref.double()).abs() / (2 * U_RND[dtype] * wp_ref.double().abs() + 2.0 ** -24)).max()) <= 1.0
    assert float(((s_vec.double() - wp.double().sum(1)).abs() / (c * NR.U32 * wp.double().abs().sum(1))).max()) <= 1.0
    assert float(((c_vec.double() - c_ref).abs() / ((c + 1) * NR.U32 * (w.double().abs() @ beta.double().abs() + bias.double().abs()))).max()) <= 1.0
    xr, stat = with_tail(x), nan_buffer(m * 2)
    capi.check(lib.etainv_op_row_stats(capi.ptr(xr), capi.ptr(stat), m, c, eps, dt, capi.stream_ptr()))
    assert_tail(stat, m * 2, "row statistics")
    st = stat[: m * 2].reshape(m, 2)
    mean, _, rstd = NR.ref_row_stats(x, eps)
    label = f"gemm_ln ({m}, {c}, {n}) {NR.NAME[dtype]}"
    assert_stats(label, st[:, 0], st[:, 1], mean, rstd, *NR.row_stats_err(x, eps))
    out = guarded(m, n, dtype)
    capi.check(lib.etainv_op_gemm_ln(capi.ptr(xr), capi.ptr(wp), capi.ptr(c_vec), capi.ptr(s_vec), capi.ptr(stat), None, capi.ptr(out), None, None, m, n, c, 0, dt,
                                     capi.stream_ptr()))
    assert_guard(out, m)
    ref, bound, e = NR.gemm_ln_bound(x, wp, c_vec, eps, dtype)
    emu = NR.emulate_gemm_ln(x, wp, s_vec, c_vec, st[:, 0], st[:, 1])
    k = NR.worst(out[:m], ref, bound)
    print(f"margin {label}: kernel {k:.3f} emulation {NR.worst(emu.to(dtype), ref, bound):.3f} (before its rounding {NR.worst(emu, ref, e):.3f} of e)")
    assert k <= 1.0, f"{label}: {offender(out[:m], ref, bound)}"
