"""CPU checks of tests/norm_ref.py: every float64 reference against torch's own group_norm / layer_norm and the oracle's modules, the Chan merge and the
sum / sum-of-squares finalize against statistics of the concatenated data, the restatement of launch_groupnorm's geometry against hand-computed cases, and the
condition that makes the GPU tests' bounds legitimate: on exactly the inputs of every GPU case the emulation -- the best the kernels' expressions can do -- uses at
most half of the part of each bound that stands in front of the output rounding, and stays inside the whole bound once rounded."""
import pytest
import torch
import torch.nn.functional as F

from tests import norm_ref as NR

HALF = 0.5


def nchw(x, h):
    b, hw, c = x.shape
    return x.double().permute(0, 2, 1).reshape(b, c, h, hw // h)


# ---------------------------------------------------------------------------------------------------------------- references
@pytest.mark.parametrize("groups,c1,c2", [(32, 320, 0), (32, 640, 320), (8, 320, 0), (64, 512, 0), (32, 1280, 640)])
@pytest.mark.parametrize("silu", [0, 1])
def test_groupnorm_reference_is_torch_group_norm(groups, c1, c2, silu):
    x = NR.gn_input(3, 24, c1 + c2, groups, torch.float16, "random", seed=1)
    gamma, beta = NR.norm_params(c1 + c2, seed=2)
    want = F.group_norm(x.double().permute(0, 2, 1), groups, gamma.double(), beta.double(), NR.f32(1e-5)).permute(0, 2, 1)
    want = F.silu(want) if silu else want
    got = NR.ref_groupnorm(torch.cat([x[..., :c1], x[..., c1:]], -1), gamma, beta, groups, 1e-5, silu)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    mean, var, rstd = NR.ref_gn_stats(x, groups, 1e-5)
    g = x.double().reshape(3, 24, groups, -1).permute(0, 2, 1, 3).reshape(3, groups, -1)
    torch.testing.assert_close(mean, g.mean(-1), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(rstd, (g.var(-1, unbiased=False) + NR.f32(1e-5)).rsqrt(), rtol=1e-12, atol=0)


def test_groupnorm_reference_is_the_oracle_modules():
    from oracle import unet as ounet
    from oracle import vae as ovae
    for norm, c, h in ((ounet.ResnetBlock2D(960, 320).norm1, 960, 4), (ovae.Res(128, 256).norm1, 128, 6), (ounet.Transformer2DModel(320, 768, 8).norm, 320, 4)):
        norm = norm.double()
        with torch.no_grad():
            norm.weight.copy_(1 + 0.1 * torch.randn(c, generator=torch.Generator().manual_seed(c)).double())
            norm.bias.copy_(0.1 * torch.randn(c, generator=torch.Generator().manual_seed(c + 1)).double())
            x = NR.gn_input(2, 24, c, 32, torch.bfloat16, "random", seed=3)
            want = norm(nchw(x, h))
            got = NR.ref_groupnorm(x, norm.weight, norm.bias, norm.num_groups, norm.eps, 0)
        # (the module holds eps as a Python float, the kernels receive it rounded to fp32: a relative 1e-8 of eps / var)
        torch.testing.assert_close(nchw(got, h), want, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("c", [8, 320, 1536])
def test_layernorm_reference_is_torch_layer_norm_and_the_oracle_module(c):
    from oracle import unet as ounet
    x = NR.row_input(7, c, torch.float16, "random", seed=c)
    gamma, beta = NR.ln_params(c)
    want = F.layer_norm(x.double(), (c,), gamma.double(), beta.double(), NR.f32(1e-5))
    torch.testing.assert_close(NR.ref_layernorm(x, gamma, beta, 1e-5), want, rtol=1e-12, atol=1e-12)
    mean, var, rstd = NR.ref_row_stats(x, 1e-5)
    torch.testing.assert_close(rstd, (x.double().var(-1, unbiased=False) + NR.f32(1e-5)).rsqrt(), rtol=1e-12, atol=0)
    if c == 320:
        blk = ounet.BasicTransformerBlock(320, 768, 8).norm1.double()
        with torch.no_grad():
            torch.testing.assert_close(NR.ref_layernorm(x, blk.weight, blk.bias, blk.eps), blk(x.double()), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("p,cw", [(1, 32), (2, 80), (10, 32), (16, 80)])
@pytest.mark.parametrize("family", NR.LNF_FAMILIES)
def test_chan_merge_is_the_statistics_of_the_concatenated_data(p, cw, family):
    """on float64 partials (the fp32 rounding of ln_partials is the hand-over's, not the merge's)"""
    g = torch.Generator().manual_seed(p * cw)
    x = torch.randn(9, p, cw, generator=g, dtype=torch.float64) * 1.5 + (10.0 * torch.arange(p).double()[None, :, None] if family == "cross" else 0.3)
    if family == "all_const":
        x[:] = 0.5
    if family == "chunk_const":
        x[:, p // 2] = 0.5
    mean = x.mean(-1)
    part = torch.stack([mean, ((x - mean[..., None]) ** 2).sum(-1)], -1)
    got_mean, got_rstd = NR.chan_merge(part, cw, 1e-5)
    want_mean, _, want_rstd = NR.ref_row_stats(x.reshape(9, p * cw), 1e-5)
    torch.testing.assert_close(got_mean, want_mean, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(got_rstd, want_rstd, rtol=1e-11, atol=0)
    # and the fp32 hand-over: the partials builder rounds exactly these
    torch.testing.assert_close(NR.ln_partials(x.reshape(9, p * cw), p).double(), part, rtol=2.0 ** -24, atol=1e-30)


@pytest.mark.parametrize("b,hw,c1,c2,wm1,wm2", NR.GN_PRE_CASES)
def test_partial_finalize_is_the_statistics_of_the_concatenated_data(b, hw, c1, c2, wm1, wm2):
    """integers: every block sum is exact in fp32, so the finalize must reproduce the two-pass statistics to float64 accuracy"""
    g = torch.Generator().manual_seed(hw + c1)
    x = torch.randint(-8, 9, (b, hw, c1 + c2), generator=g).double() * (1 + torch.arange(b).double())[:, None, None]
    gamma, beta = NR.norm_params(c1 + c2, seed=5)
    p1, p2 = NR.gn_partials(x[..., :c1], wm1), (NR.gn_partials(x[..., c1:], wm2) if c2 else None)
    assert p1.shape == (b * hw // wm1, 2, c1) and p1.dtype == torch.float32
    mean, rstd, planes = NR.gn_from_partials(p1, wm1, p2, wm2, b, hw, 32, 1e-6, gamma, beta)
    want_mean, _, want_rstd = NR.ref_gn_stats(x, 32, 1e-6)
    torch.testing.assert_close(mean, want_mean, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(rstd, want_rstd, rtol=1e-11, atol=0)
    assert planes.shape == (b, 2, c1 + c2)
    y = x * planes[:, None, 0] + planes[:, None, 1]
    torch.testing.assert_close(y, NR.ref_groupnorm(x, gamma, beta, 32, 1e-6, 0), rtol=1e-10, atol=1e-10)


# ---------------------------------------------------------------------------------------------------------------- geometry
# (b, hw, c1, c2, groups) -> what launch_groupnorm does, computed by hand from its three formulas
GEOMETRY_TABLE = [
    ((1, 520, 320, 0, 32), dict(chunks=64, per=9, empty_stats=[58, 59, 60, 61, 62, 63], chunks_apply=130, per_apply=4, empty_apply=[], chain_pixels=3,
                                stats_vpl=1, apply_mode=0, lds_adds=4 * 2 + 3)),
    ((40, 1024, 320, 0, 32), dict(chunks=25, per=41, empty_stats=[], chunks_apply=51, per_apply=21, empty_apply=[49, 50], chain_pixels=11)),
    ((1100, 16, 320, 0, 32), dict(chunks=1, per=16, chunks_apply=1, per_apply=16, chain_pixels=4, empty_stats=[], empty_apply=[])),
    ((128, 4096, 320, 0, 32), dict(chunks=8, per=512, chain_pixels=128, chunks_apply=16)),
    ((256, 1024, 320, 0, 32), dict(chunks=4, per=256, chain_pixels=64, chunks_apply=8)),
    ((2, 72, 640, 320, 32), dict(chunks=9, per=8, chunks_apply=18, per_apply=4, stats_vpl=2, apply_mode=2, cpg=30, lds_adds=4 * 4 + 3)),
    ((2, 72, 1280, 0, 32), dict(stats_vpl=3, apply_mode=3)),
    ((2, 72, 1280, 640, 32), dict(stats_vpl=4, apply_mode=4, cpg=60, lds_adds=4 * 8 + 3)),
    ((2, 72, 1280, 1280, 32), dict(stats_vpl=5, apply_mode=5)),
    ((2, 72, 640, 0, 32), dict(stats_vpl=2, apply_mode=0)),
    ((2, 72, 512, 0, 64), dict(stats_vpl=1, apply_mode=1, wide_groups=True, lds_adds=4 * 8)),
    ((2, 72, 128, 0, 32), dict(stats_vpl=1, apply_mode=1, cpg=4, lds_adds=4 * 1 + 3)),
    ((1, 7, 320, 0, 32), dict(chunks=1, per=7, chunks_apply=1, per_apply=7, chain_pixels=2)),
    ((1, 3, 1280, 0, 32), dict(chunks=1, chunks_apply=1, per=3, chain_pixels=1)),
    ((3, 9, 320, 0, 32), dict(chunks=1, per=9, chunks_apply=2, per_apply=5, chain_pixels=3)),
    ((1, 16384, 128, 0, 32), dict(chunks=64, per=256, chunks_apply=2048, per_apply=8)),
]


@pytest.mark.parametrize("args,want", GEOMETRY_TABLE)
def test_geometry_restatement(args, want):
    NR.check_premise(NR.gn_geometry(*args), want, str(args))
    geo = NR.gn_geometry(*args)
    assert geo.chain == geo.chain_pixels + 1 + geo.lds_adds


def test_geometry_noflat_and_block_count_switches():
    assert NR.gn_geometry(2, 72, 320, noflat=True).apply_mode == 1 and NR.gn_geometry(2, 72, 640, noflat=True).apply_mode == 2
    assert NR.gn_geometry(4, 4096, 320, apply_blocks=512).chunks_apply == 128


def test_every_gpu_case_states_its_premise():
    names = [c[0] for c in NR.GN_CASES]
    assert len(set(names)) == len(names)
    for name, b, hw, c1, c2, groups, family, premise in NR.GN_CASES:
        NR.check_premise(NR.gn_geometry(b, hw, c1, c2, groups), premise, name)
    reached = {(NR.gn_geometry(*c[1:6]).stats_vpl, NR.gn_geometry(*c[1:6]).apply_mode) for c in NR.GN_CASES}
    assert {s for s, _ in reached} == {1, 2, 3, 4, 5} and {a for _, a in reached} == {0, 1, 2, 3, 4, 5}
    assert {NR.gn_geometry(b, hw, c1, c2).apply_mode for b, hw, c1, c2, _, _ in NR.GN_PRE_CASES} == {0, 2, 4, 5}      # the pre_scsh form of the apply


# ---------------------------------------------------------------------------------------------------------------- the SiLU figure
def test_silu_figure():
    got = NR.measure_silu_error()
    print(f"silu emulation against float64: {got:.3f} u (1 + |y|) |silu|; the module states {NR.SILU_MEASURED}")
    assert got <= NR.SILU_MEASURED and NR.K_SILU == 2 * NR.SILU_MEASURED
    assert got > 0.5 * NR.SILU_MEASURED, "the stated figure is no longer the measured one"
    y = torch.linspace(-30, 30, 60001, dtype=torch.float64)
    yy = y.clone().requires_grad_(True)
    F.silu(yy).sum().backward()
    assert float(yy.grad.abs().max()) <= NR.SILU_LIP


# ---------------------------------------------------------------------------------------------------------------- emulation within half of every bound
def assert_half(label, arithmetic, emulation):
    print(f"{label}: emulation before its rounding {arithmetic:.3f} of e, rounded {emulation:.3f} of the bound")
    assert arithmetic <= HALF, f"{label}: the emulation alone uses {arithmetic:.3f} of the bound's arithmetic part: the bound or the input is wrong"
    assert emulation <= 1.0, label


@pytest.mark.parametrize("dtype", NR.DTYPES3, ids=NR.NAME.get)
@pytest.mark.parametrize("name", [c[0] for c in NR.GN_CASES])
def test_groupnorm_emulation_uses_half_of_the_bound(dtype, name):
    case = NR.gn_case(dtype, name)
    # the large case in two slabs of 16 images (every image scale), with the geometry of the whole batch
    slabs = [slice(0, 16), slice(case.b - 16, case.b)] if case.b * case.hw * case.c > 1 << 25 else [slice(None)]
    for sl in slabs:
        x = case.x[sl]
        for eps, silu in NR.EPS_SILU:
            r = case.evaluate(x, case.gamma, case.beta, eps, silu)
            assert_half(f"{case.label} silu {silu}", r["arithmetic"], r["emulation"])
            if dtype != torch.float32:
                # the kernel's own summation order: inside the whole bound once rounded, and inside half of the part in front of the rounding wherever the
                # bound is the conditioned one.  The two ratio8 cases are held to the bound of the CENTRED group: there the fp32 E[x^2] - mean^2 chains
                # use 0.41 .. 1.04 of that part (fp16; bf16 0.12 .. 0.25), i.e. the kernel is as good as its io type at |mean| / std = 8, not as good as fp32
                print(f"{case.label} silu {silu}: statistics in the kernel's order {r['kernel_order']:.3f} of e, rounded {r['kernel_order_rounded']:.3f} of the bound")
                assert r["kernel_order_rounded"] <= 1.0, case.label
                assert case.family == "ratio8" or r["kernel_order"] <= HALF, case.label
                # the statistics as the kernel sums them, per (image, group), inside the conditioned bound
                mean, var, rstd = NR.ref_gn_stats(x, case.groups, eps)
                dmean, drstd = NR.gn_stats_err16(x, case.groups, eps, case.geo)
                m32, r32 = NR.emulate_gn_stats16(x, case.groups, eps, case.geo)
                assert float(((m32.double() - mean).abs() / (dmean + NR.U32 * mean.abs() + 1e-300)).max()) <= HALF, case.label
                assert float(((r32.double() - rstd).abs() / (rstd * (drstd + NR.U32))).max()) <= HALF, case.label
            if case.family == "const":
                # all sums exact: beta itself without SiLU (a multiple of 1/8), silu(beta) within const_bound with it
                ref, bound, e = NR.const_bound(0.5, NR.f32(eps) ** -0.5, case.gamma, case.beta, silu, dtype)
                assert NR.worst(r["emu"], ref.expand_as(r["emu"]), e.expand_as(r["emu"]) + 1e-300) <= 1.0
                if not silu:
                    assert torch.equal(r["emu"].to(dtype).double(), case.beta.double().expand_as(r["emu"]))


@pytest.mark.parametrize("dtype", NR.DTYPES16, ids=NR.NAME.get)
@pytest.mark.parametrize("family", NR.GN_PRE_FAMILIES)
@pytest.mark.parametrize("idx", range(len(NR.GN_PRE_CASES)))
def test_groupnorm_pre_emulation_uses_half_of_the_bound(dtype, idx, family):
    case = NR.pre_case(dtype, idx, family)
    x = torch.cat([case.x1] + ([case.x2] if case.c2 else []), -1)
    for eps, silu in NR.EPS_SILU:
        r = case.evaluate(x, case.p1, case.p2, case.gamma, case.beta, eps, silu)
        assert_half(f"{case.label} silu {silu}", r["arithmetic"], r["emulation"])
        # statistics and planes of the emulation (float64 rounded to fp32, the two fp32 expressions) inside their bounds
        m32, r32 = r["mean"].float(), r["rstd"].float()
        assert float(((m32.double() - r["mean"]).abs() / (r["dmean"] + 1e-300)).max()) <= HALF
        assert float(((r32.double() - r["rstd"]).abs() / (r["rstd"] * r["drstd"])).max()) <= HALF
        sc, sh = NR.emulate_scsh(m32, r32, case.gamma, case.beta, case.c // 32)
        assert NR.worst(torch.stack([sc, sh], 1), r["planes"], r["planes_bound"] + 1e-300) <= HALF
        # the finalize of the rounded partials against the two-pass statistics of the data: the hand-over's own loss, bounded by the fp32 rounding of
        # the block sums times the condition number
        mean, var, rstd = NR.ref_gn_stats(x, 32, eps)
        cond = (mean ** 2 + var) / (var + NR.f32(eps))
        assert float(((r["rstd"] - rstd).abs() / (rstd * NR.U32 * cond)).max()) <= 1.5


@pytest.mark.parametrize("dtype", NR.DTYPES3, ids=NR.NAME.get)
@pytest.mark.parametrize("family", NR.LN_FAMILIES)
@pytest.mark.parametrize("c", NR.LN_WIDTHS)
def test_layernorm_emulation_uses_half_of_the_bound(dtype, c, family):
    if dtype == torch.float32 and c > 1280:
        return
    x = NR.row_input(max(NR.LN_ROWS), c, dtype, family, seed=c)
    gamma, beta = NR.ln_params(c)
    ref, bound, e = NR.ln_bound(x, gamma, beta, 1e-5, dtype)
    emu = NR.emulate_layernorm(x, gamma, beta, 1e-5, dtype)
    assert_half(f"layernorm c={c} {family} {NR.NAME[dtype]}", NR.worst(emu, ref, e + 1e-300), NR.worst(emu.to(dtype), ref, bound))
    mean, var, rstd = NR.ref_row_stats(x, 1e-5)
    dmean, drstd = NR.row_stats_err(x, 1e-5)
    m32, r32 = NR.emulate_row_stats(x, 1e-5, dtype)
    assert float(((m32.double() - mean).abs() / dmean).max()) <= HALF
    assert float(((r32.double() - rstd).abs() / (rstd * drstd)).max()) <= HALF
    if family == "const_row":
        rows = NR.const_rows(x.shape[0])
        assert torch.equal(emu[rows].to(dtype), beta.to(dtype)[None].expand(len(rows), c)), "a constant row normalises to beta exactly"
        assert torch.equal(m32[rows].double(), x[rows, 0].double())


@pytest.mark.parametrize("family", NR.LNF_FAMILIES)
@pytest.mark.parametrize("cw", NR.LNF_CW)
@pytest.mark.parametrize("p", NR.LNF_P)
def test_ln_finalize_emulation_uses_half_of_the_bound(p, cw, family):
    part = NR.lnf_partials(max(NR.LNF_ROWS), p, cw, family, seed=p + cw)
    mean, rstd = NR.chan_merge(part, cw, 1e-5)
    dmean, drstd = NR.ln_finalize_err(part, cw, 1e-5)
    m32, r32 = NR.emulate_ln_finalize(part, cw, 1e-5)
    a, b = float(((m32.double() - mean).abs() / (dmean + 1e-300)).max()), float(((r32.double() - rstd).abs() / (rstd * drstd)).max())
    print(f"ln_finalize P={p} cw={cw} {family}: emulation mean {a:.3f}, rstd {b:.3f} of the bound")
    assert a <= HALF and b <= HALF
    if family == "cross" and p > 1:
        var = 1 / rstd ** 2
        within = part[:, :, 1].double().sum(1) / (p * cw)
        assert float((within / var).max()) < 0.01, "the cross term carries (almost) all of the variance"
    if family == "all_const":
        assert float((rstd * NR.f32(1e-5) ** 0.5 - 1).abs().max()) < 1e-12


@pytest.mark.parametrize("dtype", NR.DTYPES16, ids=NR.NAME.get)
@pytest.mark.parametrize("m,c,n", NR.GEMM_LN_CASES)
def test_gemm_ln_emulation_uses_half_of_the_bound(dtype, m, c, n):
    x, w, gamma, beta, bias = NR.gemm_ln_inputs(m, c, n, dtype)
    mean, var, rstd = NR.ref_row_stats(x, 1e-5)
    assert 7.0 < float((mean.abs() * var.rsqrt()).min()) and float((mean.abs() * var.rsqrt()).max()) < 9.0
    wp, s_vec, c_vec = NR.fold_ref(w, gamma, beta, bias, dtype)
    ref, bound, e = NR.gemm_ln_bound(x, wp, c_vec, 1e-5, dtype)
    # the reference IS float64 LayerNorm(x) W'^T + b
    want = F.layer_norm(x.double(), (c,), gamma.double(), beta.double(), NR.f32(1e-5)) @ (wp.double() / gamma.double()).t() + bias.double()
    drift = (w.double() - wp.double() / gamma.double()).abs() @ beta.double().abs()          # beta meets the unrounded W in c = W beta + bias
    assert float(((ref - want).abs() - drift[None]).max()) < 1e-9
    m32, r32 = NR.emulate_row_stats(x, 1e-5, dtype)
    emu = NR.emulate_gemm_ln(x, wp, s_vec.float(), c_vec.float(), m32, r32)
    assert_half(f"gemm_ln ({m}, {c}, {n}) {NR.NAME[dtype]}", NR.worst(emu, ref, e), NR.worst(emu.to(dtype), ref, bound))
