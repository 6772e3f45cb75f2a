"""tests/gemm_ref.py on the CPU: the references against torch's own convolution, the layout maps, the premises of the case list, the condition under which its
bounds mean anything (an fp32 emulation uses at most half of them on exactly the inputs the GPU test uses), the conditions of the exact-integer family, and
the evidence that both families can fail: an emulation broken one way at a time.  References and emulations are evaluated on a sample of the output rows of
the large cases (Case.sample_rows: the operands are the whole case's)."""
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_ref as G

ROWS = 320
CONV_FORMS = [c for c in G.CASES if c.kind == "conv"]


def small(case, images=2):
    """the same conv at `images` images"""
    return G.Case(case.name + "@2", "conv", tuple(case.plan.values()), case.entry, n=case.n, k1=case.k1, k2=case.k2, images=images, h=case.h, w=case.w,
                  stride=case.stride, ups=case.ups, pad0=case.pad0)


def conv2d64(case, x, w_oc33):
    """F.conv2d in float64 on the CPU: x [b][h][w][c], w [n][c][3][3] -> [m][n]"""
    x = x.double().reshape(case.images, case.h, case.w, -1).permute(0, 3, 1, 2)
    if case.ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    if case.pad0:
        y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w_oc33.double(), stride=2, padding=0)
    else:
        y = F.conv2d(x, w_oc33.double(), stride=case.stride, padding=1)
    return y.permute(0, 2, 3, 1).reshape(case.m, case.n)


@pytest.mark.parametrize("name", sorted({c.name for c in CONV_FORMS}))
def test_conv_references_agree_with_conv2d(name):
    case = small(G.CASE[name])
    g = torch.Generator().manual_seed(1)
    x = torch.randn(case.images * case.h * case.w, case.k1 + case.k2, generator=g, dtype=torch.float64)
    w33 = torch.randn(case.n, case.k1 + case.k2, 3, 3, generator=g, dtype=torch.float64)
    want = conv2d64(case, x, w33)
    if case.ups == 2:
        # the phase form on the unrounded sums of the fp32 originals equals the nine-tap form
        acc, _ = G.accumulate(case, x, None, G.pack_ups4_ref(w33, None), torch.float64)
        nine = G.Case("nine", "conv", tuple(G.CASE["ups9"].plan.values()), "conv", n=case.n, k1=case.k1, images=case.images, h=case.h, w=case.w, ups=1)
        acc9, _ = G.accumulate(nine, x, None, w33.permute(0, 2, 3, 1).contiguous(), torch.float64)
        assert float((acc - acc9).abs().max()) <= 1e-12 * float(acc9.abs().max())
    else:
        acc, ab = G.accumulate(case, x, None, w33.permute(0, 2, 3, 1).contiguous(), torch.float64)
        assert bool((ab >= acc.abs() - 1e-12).all())
    assert float((acc - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_a_sample_of_rows_is_the_rows_of_the_whole():
    case = small(G.CASE["ring-stride2"])
    o = G.case_operands(case, torch.float16, "random")
    full, _ = G.accumulate(case, o.a1, None, o.w, torch.float64)
    rows = torch.tensor([0, 5, 255, 256, 511])
    part, _ = G.accumulate(case, o.a1, None, o.w, torch.float64, rows)
    assert torch.equal(part, full[rows])


def test_pack_ups4_sums_the_taps_that_share_a_source_pixel():
    w = torch.arange(2 * 3 * 9, dtype=torch.float64).reshape(2, 3, 3, 3)
    p = G.pack_ups4_ref(w, None)                               # [phase][cout][tap][cin]
    assert torch.equal(p[0, :, 0], w[:, :, 0, 0]) and torch.equal(p[0, :, 3], w[:, :, 1:, 1:].sum((2, 3)))
    assert torch.equal(p[3, :, 0], w[:, :, :2, :2].sum((2, 3))) and torch.equal(p[3, :, 3], w[:, :, 2, 2])
    assert torch.equal(p.sum((0, 2)), 4 * w.sum((2, 3)))          # every 3 x 3 tap lands in each phase exactly once


@pytest.mark.parametrize("m,n,dim,tokens", [(512, 960, 40, 256), (1024, 1920, 80, 512)])
def test_head_major_map_is_a_bijection(m, n, dim, tokens):
    idx = G.hm_index(m, n, 8, dim, tokens)
    assert torch.equal(idx.flatten().sort().values, torch.arange(m * n))
    # q of row 0, head 0: tokens x dim contiguous; the k plane starts after all rows' q
    assert int(idx[1, 0]) == dim and int(idx[0, dim]) == tokens * dim and int(idx[0, 8 * dim]) == m * 8 * dim


def test_patch_rows_enumerate_every_pixel_patch_by_patch():
    idx = G.patch_rows(2, 32, 48)
    assert torch.equal(idx.sort().values, torch.arange(2 * 32 * 48))
    assert idx[:16].tolist() == list(range(16)) and int(idx[16]) == 48 and int(idx[256]) == 16 and int(idx[3 * 256]) == 16 * 48
    assert torch.equal(G.patch_rows(3, 16, 16), torch.arange(3 * 256))                      # one patch per image: the NHWC order itself


def test_geglu_split_follows_the_packing():
    n = 256
    logical = torch.arange(n).float()[:, None]                                  # logical row r of a weight = r
    phys = G.pack_geglu(logical)[:, 0][None, :]                                 # [1][n] physical order
    a, g = G.geglu_split(phys)
    assert torch.equal(a[0], torch.arange(n // 2).float()) and torch.equal(g[0], torch.arange(n // 2, n).float())


def test_erf_constant_is_the_measured_one():
    got = G.measure_erf_error()
    assert 0.99 * G.ERF_MEASURED <= got <= G.ERF_MEASURED, got
    assert got <= 1.8e-7, "csrc/common.h claims 1.8e-7"
    x = torch.linspace(-6, 6, 200001, dtype=torch.float64)
    d = 0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-x * x / 2) / (2 * torch.pi) ** 0.5
    assert float(d.abs().max()) <= G.GELU_LIP
    assert float((G.gelu_pair_emu(x).double() - G.gelu64(x.float())).abs().max()) <= 0.5 * 6 * G.ERF_ERR + 2 * G.U32 * 6


def test_the_case_list_meets_the_dispatch_rule():
    for case in G.CASES:
        for dtype in case.dtypes():
            assert G.route_rule(case, dtype) == case.plan_for(dtype), f"{case.name} {G.NAME[dtype]}: the rule gives {G.route_rule(case, dtype)}"
        if case.lnprod or case.gnprod:
            assert case.n % G.LN_CHUNK == 0 and case.rows_per_image % G.GN_ROWS == 0
    # what the table of the cases is for: every route, every two-slot tile with and without a split, both ppconv forms, every dual-N kind
    plans = {tuple(c.plan.values()) for c in G.CASES}
    assert {p[0] for p in plans} == set(G.ROUTES) - {"fp32"}
    assert {(p[1], p[2], p[3] > 1) for p in plans if p[0] == "two-slot"} >= {(64, 64, False), (64, 64, True), (128, 160, False), (128, 160, True), (128, 128, False)}
    assert {p[4] for p in plans if p[0] == "dualn"} == {0, 1, 2, 3} and {p[4] for p in plans if p[0] == "ppconv"} == {0, 1}
    # the fp32 twin refuses the fused LayerNorm / GroupNorm forms
    assert G.route_rule(G.CASE["ts64-splitk-ln"], torch.float32) is None


@pytest.mark.parametrize("param", G.PARAMS, ids=G.param_id)
def test_emulation_uses_half_of_the_bound(param):
    """a condition on the INPUTS: where it fails, the inputs change, not the bound"""
    name, dtype, family = param
    case = G.CASE[name]
    o = G.case_operands(case, dtype, family)
    rows = case.sample_rows(ROWS)
    ref, bound, e = G.reference(case, o, dtype, case.plan_for(dtype)["ksplit"], rows)
    emu = G.emulate(case, o, rows)
    out_t = torch.float32 if case.f32out else dtype
    if family == "exact":
        assert float(ref.abs().max()) <= 256 and 64 * float(ref.abs().max()) ** 2 < 2 ** 24
        assert torch.equal(ref.to(out_t).double(), ref), "a reference value the stored type does not hold"
        assert torch.equal(emu.double(), ref), "integer operands: fp32 is exact in any order"
        return
    assert G.worst(emu, ref, e) <= 0.5, f"{name}: the fp32 emulation uses {G.worst(emu, ref, e):.3f} of e"
    assert G.worst(emu.to(out_t), ref, bound) <= 1.0


def _differs(t, dim):
    """every slice along `dim` differs from the next one"""
    t = t.movedim(dim, 0).flatten(1)
    return bool((t[1:] != t[:-1]).any(1).all())


@pytest.mark.parametrize("name", [c.name for c in G.CASES if not c.geglu])
def test_exact_operands_differ_from_their_neighbours(name):
    case = G.CASE[name]
    o = G.case_operands(case, torch.bfloat16, "exact")
    a = o.a.float()
    assert set(a.unique().tolist()) <= {-1.0, 0.0, 1.0} and set(o.w.float().unique().tolist()) <= ({-1.0, 0.0, 1.0} if case.ups != 2 else set(range(-4, 5)))
    assert _differs(a, 0), "neighbouring activation rows (pixels, and images at their seam)"
    assert _differs(a.reshape(a.shape[0], -1, 64), 1), "neighbouring K tiles of the activations"
    assert _differs(a.reshape(case.images, -1), 0) if case.images > 1 else True
    w = o.w.float()
    if case.ups == 2:
        assert _differs(w, 0) and _differs(w, 1) and _differs(w, 2)                    # phases, output channels, taps
    elif case.per_image:
        wv = w.reshape(case.images, case.n, -1)
        assert _differs(wv, 0) and _differs(wv, 1)
        assert bool((o.bias[1:] != o.bias[:-1]).all())                                 # the next image's bias differs in every column
    else:
        assert _differs(w, 0) and _differs(w, 1), "neighbouring output channels and taps"
        assert _differs(w.reshape(case.n, -1, 64), 1), "neighbouring K tiles of the weights"
    bias = o.bias.reshape(-1, case.n)
    assert bool((bias[:, 1:] != bias[:, :-1]).all()) and float(bias.abs().max()) <= 8
    assert bool((o.time[:, 1:] != o.time[:, :-1]).all()) and (case.images == 1 or bool((o.time[1:] != o.time[:-1]).all())) and float(o.time.abs().max()) <= 8
    res = o.res.float()
    assert bool((res[:, 1:] != res[:, :-1]).all()) and (case.m == 1 or bool((res[1:] != res[:-1]).all())) and float(res.abs().max()) <= 16
    for step in (16, 64, 80, 160, 256):                                                # a tile further on
        assert bool((bias[:, step:] != bias[:, :-step]).all()) and bool((res[:, step:] != res[:, :-step]).all())
        if case.m > step:
            assert bool((res[step:] != res[:-step]).all())
    st = o.stat
    assert bool((st[1:] != st[:-1]).all()) and bool((st[:, 0] == st[:, 0].round()).all()) and bool((torch.log2(st[:, 1]) % 1 == 0).all())
    assert bool((o.s[1:] != o.s[:-1]).all())


FAULT_CASES = {"ulp2": "ts64-splitk-time", "bias": "ts64-splitk-time", "res": "ts64-splitk-time", "stat": "ts64-splitk-ln", "ktile": "ts64-splitk-ln",
               "tap": "f32-stride2"}


@pytest.mark.parametrize("dtype", G.DTYPES16, ids=G.NAME.get)
@pytest.mark.parametrize("fault", list(FAULT_CASES))
def test_a_broken_emulation_fails_both_families(fault, dtype):
    """the element of largest magnitude off by two ulps of the stored type, the bias of column n + 1, the residual of row m + 1, the stat row m + 1, one K tile dropped, a conv tap
    shifted by one pixel at the top border -- on 64 rows x the columns of one wave tile.  random: outside the bound at (nearly) every broken element whose
    value the fault changes by more than the bound, and nowhere else; exact: unequal at every broken element that the fault changes at all"""
    case = G.CASE[FAULT_CASES[fault]]
    rows = case.sample_rows(ROWS)
    sel = (slice(0, 64), slice(32, 64))
    for family in G.FAMILIES:
        o = G.case_operands(case, dtype, family)
        ref, bound, e = G.reference(case, o, dtype, case.plan["ksplit"], rows)
        good = G.emulate(case, o, rows).to(dtype)
        if fault == "ulp2":
            bad = good.clone()
            at = divmod(int(ref.abs().argmax()), ref.shape[1])      # where the output rounding, not the accumulation, is most of the bound
            v = bad[at]
            ulp = 2.0 ** (torch.frexp(v.float().abs())[1].item() - 1 - (10 if dtype == torch.float16 else 7))
            bad[at] = v.float() + 2 * ulp * (1 if float(v) >= float(ref[at]) else -1)        # away from the reference
            broken = torch.zeros_like(good, dtype=torch.bool)
            broken[at] = True
        else:
            bad = good.clone()
            bad[sel] = G.emulate(case, o, rows, fault=fault).to(dtype)[sel]
            broken = bad != good
            assert int(broken.sum()) >= (8 if fault == "tap" else 1000), "the fault must reach the output"
        outside = (bad.double() - ref).abs() > bound
        assert not bool((outside & ~broken).any())
        if family == "exact":
            assert torch.equal(good.double(), ref) and bool((bad.double() != ref)[broken].all()) and not torch.equal(bad.double(), ref)
        else:
            if fault == "ulp2":
                assert bool(outside[at])
                continue
            moved = (bad.double() - good.double()).abs() > 2 * bound
            assert int(moved.sum()) >= 0.5 * int(broken.sum()) and bool(outside[moved].all())


def test_partial_bounds_hold_for_an_fp32_emulation_in_the_kernels_order():
    """LayerNorm partials: lane fq of a row holds columns 16 j + 4 fq + q of its 80-column chunk; lanes (0, 1) and (2, 3) merge, then the halves.
    GroupNorm partials: 64 rows summed in fp32 one after the other.  Both within half of their bounds"""
    g = torch.Generator().manual_seed(5)
    for dtype in G.DTYPES16:
        x = ((torch.randn(256, 320, generator=g) * 1.5 + 0.7) * (1 + torch.arange(256) % 16).float()[:, None]).to(dtype)
        ch = x.float().reshape(256, 4, 5, 4, 4).permute(0, 1, 3, 2, 4).reshape(256, 4, 4, 20)          # [row][chunk][lane fq][20]
        s = torch.zeros(256, 4, 4)
        for i in range(20):
            s = s + ch[..., i]
        mu = s * torch.tensor(1.0 / 20.0)
        m2 = torch.zeros_like(mu)
        for i in range(20):
            d = ch[..., i] - mu
            m2 = m2 + d * d
        n = 20.0
        for _ in range(2):
            d = mu[..., 1::2] - mu[..., 0::2]
            m2 = m2[..., 0::2] + (m2[..., 1::2] + d * d * (0.5 * n))
            mu = mu[..., 0::2] + 0.5 * d
            n *= 2
        want, (dm, dq) = G.ln_partials64(x), G.ln_partial_err(x)
        assert float(((mu[..., 0].double() - want[..., 0]).abs() / dm).max()) <= 0.5
        assert float(((m2[..., 0].double() - want[..., 1]).abs() / dq).max()) <= 0.5
        sm, sq = torch.zeros(4, 320), torch.zeros(4, 320)
        xf = x.float().reshape(4, 64, 320)
        for i in range(64):
            sm, sq = sm + xf[:, i], sq + xf[:, i] * xf[:, i]
        want, err = G.gn_partials64(x), G.gn_partial_err(x)
        assert float(((torch.stack([sm, sq], 1).double() - want).abs() / err.clamp_min(1e-300)).max()) <= 0.5
