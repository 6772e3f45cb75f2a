"""Per-block UNet parity on MI355X: every block of etainv_unet_forward, tapped (etainv_engine_set_tap), against the float64 oracle block run on the
engine's OWN tapped inputs (tests/unet_blocks_ref.py), bounded by the reference-precision floor of that block.

Shapes: `cfg32` = L 32, 8 latents twice (16 UNet rows, CFG), t = 500: the fused LayerNorm / GroupNorm paths and their producers run unsplit and the
QKV planes are head-major (asserted); `t16` = L 16, 4 rows over 4 latents at timesteps (0, 20, 500, 981) with 4 contexts: split-K and two-slot
fallbacks, the ragged 4-token level, one time-projection row per batch row.  Weights load_synthetic(0) against build_unet(0).

Bound: each of the three statistics of block_stats (global rel L2; worst row / (row, channel) slice; worst element over the tensor RMS) is at
most MARGIN = 2 times the same statistic of the floor: the emulated 16-bit execution of the block (oracle/lowprec.py: parameters rounded once,
every operator's output rounded) against float64 on the oracle's own free-running activations rounded to the dtype; for the fp32 engine the fp32
oracle block against float64.  The floors are committed (leg_block_floors, tests/golden/oracle_cache/), never measured from the engine.  The engine
rounds less often than the emulation (fp32 accumulators, fused norms), so it is expected below 1; 2 allows for another summation order and for the
cancellation in the LayerNorm fold rstd * (acc - mean * s).

The float64 reference runs through torch on the device: test_float64_reference_agrees_between_host_and_device holds one toy-width block of each
kind to 1e-12 between host and device first (measured 1e-15 to 4e-15).  All rows of both shapes are referenced; the module takes 20 s on the
device, none of it a host reference.

time_embedding under the fp32 engine: sin / cos of t * freq is conditioned by t (an fp32 argument near 981 carries 6e-5 of rounding), so any fp32
evaluation of the sinusoid, the oracle's and the engine's alike, is 1e-5 off the truth.  Against the oracle's own fp32 sinusoid the engine's
time_embedding measured 5.8 (cfg32) and 22 (t16) times a floor that did not contain that term; reference and floor of this point therefore take the
sinusoid in float64 (unet_blocks_ref.timestep_embedding64) when the compute dtype is fp32, and the engine sits at 1.08 / 1.14 of the floor.  The
16-bit engines round the sinusoid to 16 bits, and so do their reference and floor.

Measured (MI355X), statistic / floor.  Largest per shape and dtype, with the tap that holds it:
  cfg32 fp16  a 1.00 (down_blocks.1.downsamplers.0), b 1.02 (down_blocks.2.downsamplers.0), c 1.27 (mid_block.resnets.0); smallest 0.35
  cfg32 bf16  a 1.00 (conv_in), b 1.11 (down_blocks.2.downsamplers.0), c 1.31 (up_blocks.3.resnets.0); smallest 0.34
  cfg32 fp32  a 1.04 (down_blocks.2.downsamplers.0), b 1.38 (mid_block.resnets.0), c 1.64 (up_blocks.2.upsamplers.0); smallest 0.29
  t16   fp16  a 1.01 (down_blocks.2.downsamplers.0), b 1.07 (down_blocks.1.downsamplers.0), c 1.52 (up_blocks.1.resnets.2); smallest 0.32
  t16   bf16  a 1.00 (down_blocks.0.downsamplers.0), b 1.17 (down_blocks.1.downsamplers.0), c 1.37 (down_blocks.2.downsamplers.0); smallest 0.37
  t16   fp32  a 1.04 (down_blocks.2.downsamplers.0), b 1.17 (up_blocks.1.upsamplers.0), c 2.04 (down_blocks.2.downsamplers.0: own margin, MARGINS); smallest 0.28
Largest of (a, b, c) / floor per kind of block:
                    cfg32 fp16  cfg32 bf16  cfg32 fp32    t16 fp16    t16 bf16    t16 fp32
  time_embedding          1.00        1.00        1.08        1.00        1.00        1.14
  conv_in                 1.00        1.00        1.02        1.00        1.00        1.27
  resnets                 1.27        1.31        1.38        1.52        1.20        1.17
  attentions              1.08        1.11        0.85        0.97        1.11        0.82
  downsamplers            1.02        1.11        1.37        1.07        1.37        2.04
  upsamplers              1.12        1.00        1.64        1.14        1.21        1.22
  conv_norm_out           0.49        0.49        0.95        0.49        0.51        1.48
Global rel L2 (a), teacher-forced / free-running against one float64 oracle forward from the same inputs, largest over the taps:
fp16 4.9e-4 / 1.4e-3, bf16 4.0e-3 / 1.1e-2, fp32 5.7e-6 (time_embedding; 2.8e-7 elsewhere) / 5.2e-6 at both shapes.  The test prints the full
per-tap table.
"""
import os

import pytest
import torch

from tests import unet_blocks_ref as ub
from tests.oracle_cache import lowprec_unet, oracle_leg, oracle_unet

pytestmark = pytest.mark.gpu

MARGIN = 2.0
# (dtype name, case, tap name) -> its own margins for (a, b, c), each with its measured value and cause:
#   fp32 / t16 / down_blocks.2.downsamplers.0, statistic (c) only: measured 2.04 with (a) 1.04 and (b) 1.16.  The tensor has 4 x 4 x 1280 = 20480
#   elements, each an fp32 sum over K = 9 x 1280 = 11520 products; (c) is the single largest of 20480 rounding errors and is heavy-tailed (in the
#   floor itself it is 6.9 times the RMS error, here 13): the engine's fp32 MFMA adds along K in one dependent chain, the host GEMM of the floor in
#   blocked partial sums, so the two maxima are independent draws from such a tail while the mean error is the same ((a) at 1.04).  No systematic
#   term: a dropped bias, a wrong row or eps moves (c) by 30 to 160 times the floor (tests/test_unet_blocks_ref.py).  3 = 1.5 x the common margin.
MARGINS = {("fp32", "t16", "down_blocks.2.downsamplers.0"): (2.0, 2.0, 3.0)}
CASES = ("cfg32", "t16")
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
_memo = {}


def case_inputs(case):
    """(L, latent (n_lat, 4, L, L), ctx (rows, 77, 768), t (rows,)) of a shape, from seeds"""
    if case == "cfg32":
        g = torch.Generator().manual_seed(3201)
        return 32, torch.randn(8, 4, 32, 32, generator=g), torch.randn(16, 77, 768, generator=g), torch.full((16,), 500)
    g = torch.Generator().manual_seed(1601)
    return 16, torch.randn(4, 4, 16, 16, generator=g), torch.randn(4, 77, 768, generator=g), torch.tensor([0, 20, 500, 981])


def sample_of(latent, rows):
    return torch.cat([latent] * (rows // latent.shape[0]))                  # UNet row r reads latent r % n_lat


def oracle64():
    if "u64" not in _memo:
        from oracle.unet import build_unet
        _memo["u64"] = build_unet(0).double()
    return _memo["u64"]


def free_run(case):
    """the float64 oracle's own activations at every tap point, one forward from the fp32 inputs"""
    if ("free", case) not in _memo:
        _, latent, ctx, t = case_inputs(case)
        u = oracle64()
        _memo["free", case] = ub.capture(u, lambda: u(sample_of(latent, len(t)).double(), t, encoder_hidden_states=ctx.double()))
    return _memo["free", case]


@oracle_leg(cases=[(c, d) for c in CASES for d in DTYPES.values()])
def leg_block_floors(case, dtype):
    """{tap name: [a, b, c]}: block_stats of the reference-precision execution of each block against float64 (block_floor)"""
    _, latent, ctx, t = case_inputs(case)
    acts, u64 = free_run(case), oracle64()
    low = oracle_unet() if dtype == torch.float32 else lowprec_unet(dtype)
    smp = sample_of(latent, len(t))
    return {"floors": {n: list(ub.block_floor(low, u64, n, acts, ctx, t, smp, dtype)) for n in ub.tap_names(u64)}}


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def engines():
    from etainv.engine import Engine
    made = {}

    def get(dtype, L, batch=16):
        key = (dtype, L, batch)
        if key not in made:
            e = Engine(dtype=dtype, max_unet_batch=batch, latent_size=L, max_img=2)
            e.load_synthetic(0)
            made[key] = e
        return made[key]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def unet64_dev():
    from oracle.unet import build_unet
    u = build_unet(0).double().cuda()
    yield u
    del u
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def free_dev(unet64_dev):
    """free-running float64 activations on the device, one forward per shape (shared by the dtypes)"""
    made = {}

    def get(case):
        if case not in made:
            _, latent, ctx, t = case_inputs(case)
            smp = sample_of(latent, len(t)).double().cuda()
            with torch.device("cuda"):                                       # (the oracle's sinusoidal embedding allocates on the default device)
                made[case] = ub.capture(unet64_dev, lambda: unet64_dev(smp, t.cuda(), encoder_hidden_states=ctx.double().cuda()))
        return made[case]
    return get


def tapped_forward(e, latent, t, ctx, ctrl=None):
    with e.tapped() as taps:
        out = e.unet(latent, t, ctx, ctrl).clone()
        torch.cuda.synchronize()
        return out, taps()


# ------------------------------------------------------------------------------------------------ premises
def test_float64_reference_agrees_between_host_and_device():
    """where the float64 reference may run: a toy-width resnet, transformer, down- and upsampler, the time MLP and conv_norm_out agree between
    torch's host and device float64 to 1e-12 (largest element error over the tensor RMS)"""
    from oracle.unet import build_unet
    host = build_unet(0, block_out_channels=(64, 128, 128, 128), groups=8, heads=4, cross_dim=32).double()
    g = torch.Generator().manual_seed(2)
    smp, ctx, t = torch.randn(3, 4, 16, 16, generator=g).double(), torch.randn(3, 77, 32, generator=g).double(), torch.tensor([0, 500, 981])
    taps = ub.capture(host, lambda: host(smp, t, encoder_hidden_states=ctx))
    import copy
    dev = copy.deepcopy(host).cuda()
    for n in ("time_embedding", "conv_in", "down_blocks.0.resnets.0", "down_blocks.0.attentions.0", "down_blocks.0.downsamplers.0", "mid_block.attentions.0",
              "up_blocks.0.resnets.2", "up_blocks.1.upsamplers.0", "up_blocks.3.attentions.2", "conv_norm_out"):
        on_dev = ub.block_reference(dev, n, taps, ctx, t, smp, emb_dtype=None)       # (None: the sinusoid as the hooked host forward took it)
        err = ub.block_stats(on_dev.cpu(), taps[n])[2]
        print(f"{n}: host vs device float64 {err:.1e}")
        assert err <= 1e-12, n


def test_tap_names_are_the_oracle_modules(engines):
    e = engines(torch.float16, 16)
    with torch.device("meta"):
        from oracle.unet import UNet2DConditionModel
        u = UNet2DConditionModel()
    assert e.tap_names() == ub.tap_names(u)
    side = {n: s for n, s, _ in e.tap_specs()}
    ch = {n: c for n, _, c in e.tap_specs()}
    assert (side["time_embedding"], ch["time_embedding"]) == (1, 1280) and (side["conv_norm_out"], ch["conv_norm_out"]) == (16, 320)
    assert (side["mid_block.attentions.0"], ch["mid_block.attentions.0"]) == (2, 1280) and (side["up_blocks.2.upsamplers.0"], ch["up_blocks.2.upsamplers.0"]) == (16, 640)
    for n in e.tap_names():
        if n not in ("time_embedding", "conv_in", "conv_norm_out"):
            m = u.get_submodule(n)
            assert ch[n] == (m.conv2.out_channels if ".resnets." in n else m.proj_out.out_channels if ".attentions." in n else m.conv.out_channels), n


def test_tap_refusals_and_rows(engines):
    """a buffer smaller than max_unet_batch rows is refused when it is set (never inside a forward); NULL clears; bad points are errors"""
    from etainv import _capi
    e = engines(torch.float16, 16)
    n_tap = e.lib.etainv_engine_tap_count(e.h)
    assert n_tap == len(e.tap_names()) == 47
    i = e.tap_names().index("down_blocks.1.attentions.0")            # (8 x 8, 640 channels)
    need = 16 * 64 * 640 * 2
    buf = torch.zeros(need // 2, dtype=torch.float16, device="cuda")
    assert e.lib.etainv_engine_set_tap(e.h, i, _capi.ptr(buf), need - 1) != 0 and b"smaller" in e.lib.etainv_last_error()
    assert e.lib.etainv_engine_set_tap(e.h, n_tap, _capi.ptr(buf), need) != 0 and e.lib.etainv_engine_set_tap(e.h, -1, None, 0) != 0
    assert e.lib.etainv_engine_tap_rows(e.h, n_tap) == -1
    g = torch.Generator().manual_seed(4)
    x, ctx = torch.randn(2, 4, 16, 16, generator=g).cuda(), torch.randn(4, 77, 768, generator=g).cuda()
    ref = e.unet(x, 300, ctx).clone()
    torch.cuda.synchronize()
    assert not buf.any()                                              # the refused tap was not set
    _capi.check(e.lib.etainv_engine_set_tap(e.h, i, _capi.ptr(buf), need))
    try:
        assert torch.equal(e.unet(x, 300, ctx), ref)
        torch.cuda.synchronize()
        assert e.tap_rows("down_blocks.1.attentions.0") == 4 and buf[:4 * 64 * 640].any() and not buf[4 * 64 * 640:].any()
    finally:
        _capi.check(e.lib.etainv_engine_set_tap(e.h, i, None, 0))
    buf.zero_()
    assert torch.equal(e.unet(x, 300, ctx), ref)
    torch.cuda.synchronize()
    assert not buf.any()                                              # cleared: nothing is copied any more
    with pytest.raises(KeyError):
        with e.tapped(["no_such_block"]):
            pass


# ------------------------------------------------------------------------------------------------ the per-block bound
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("case", CASES)
def test_every_block_within_margin_of_the_floor(engines, unet64_dev, free_dev, case, dname):
    dtype = DTYPES[dname]
    L, latent, ctx, t = case_inputs(case)
    rows = len(t)
    e = engines(dtype, L)
    hm0 = e.qkv_head_major_launches
    lat_d, ctx_d = latent.cuda(), ctx.cuda()
    plain = e.unet(lat_d, t, ctx_d).clone()
    out, taps = tapped_forward(e, lat_d, t, ctx_d)
    assert torch.equal(out, plain), "setting taps changed the forward's result"
    assert torch.equal(e.unet(lat_d, t, ctx_d), plain)
    if case == "cfg32" and dtype != torch.float32:
        assert e.qkv_head_major_launches > hm0, "premise: the head-major QKV planes are on the path at this shape"
    names = ub.tap_names(unet64_dev)
    assert list(taps) == names and all(v.dtype == dtype and v.shape[0] == rows and torch.isfinite(v).all() for v in taps.values())
    ctx_r, smp_r = ctx_d.to(dtype), sample_of(lat_d, rows).to(dtype)              # what the engine computes on: inputs rounded to the compute dtype
    floors = leg_block_floors(case, dtype)["floors"]
    free = free_dev(case)
    stats, free_l2 = {}, {}
    for n in names:
        ref = ub.block_reference(unet64_dev, n, taps, ctx_r, t, smp_r)
        stats[n] = ub.block_stats(taps[n], ref)
        free_l2[n] = float((taps[n].double() - free[n]).norm() / free[n].norm())
        del ref
    ratios = ub.block_ratios(stats, floors)
    print("\n" + ub.format_table(f"{case} {dname}: teacher-forced statistics, their ratios to the floor, free-running rel L2", names,
                                 ["a", "b", "c", "a/floor", "b/floor", "c/floor", "free L2"], lambda n: (*stats[n], *ratios[n], free_l2[n])))
    worst = max(names, key=lambda n: max(ratios[n]))
    print(f"{case} {dname}: max ratio {max(ratios[worst]):.3f} at {worst}; max free-running rel L2 {max(free_l2.values()):.2e}")
    own = {n: m for (d, c, n), m in MARGINS.items() if d == dname and c == case}
    bad = [n for n in names if any(r > m for r, m in zip(ratios[n], own.get(n, (MARGIN,) * 3)))]
    assert not bad, {n: ratios[n] for n in bad}


# ------------------------------------------------------------------------------------------------ layout equalities, bit for bit at every tap
def _ptp_inputs(n=2, L=16):
    g = torch.Generator().manual_seed(33)
    x = torch.randn(2 * n, 4, L, L, generator=g).cuda()                       # [src.., tgt..]
    ctx = torch.randn(4 * n, 77, 768, generator=g).cuda()                     # [u_s, u_t, c_s, c_t]
    return x, ctx


@pytest.fixture()
def no_splitk():
    os.environ["ETAINV_NO_SPLITK"] = "1"                                       # (split-K part counts follow the row count: pinned for bit equality)
    yield
    os.environ.pop("ETAINV_NO_SPLITK", None)
    os.environ.pop("ETAINV_NO_PREFIX_SHARE", None)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_shared_prefix_equals_the_unshared_execution_at_every_tap(engines, no_splitk, dtype):
    e = engines(dtype, 16)
    x, ctx = _ptp_inputs()
    shared, taps_s = tapped_forward(e, x, 481, ctx)
    os.environ["ETAINV_NO_PREFIX_SHARE"] = "1"
    full, taps_f = tapped_forward(e, x, 481, ctx)
    assert torch.equal(shared, full)
    for n in taps_s:
        assert taps_s[n].shape == taps_f[n].shape and torch.equal(taps_s[n], taps_f[n]), n
    first = taps_s["down_blocks.0.resnets.0"]
    assert torch.equal(first[:4], first[4:]) and not torch.equal(taps_s["down_blocks.0.attentions.0"][:4], taps_s["down_blocks.0.attentions.0"][4:])


def test_three_row_and_early_exit_calls_equal_the_full_call_at_every_tap(engines, no_splitk):
    """prompt-to-prompt without the uncond source rows (first_row = n_img) against the matching rows of the four-row call, and a src_exit_block call
    against the three-row call: the rows that do not depend on the layout are bit-equal at every tap (fp32 engine: its kernels do not pick their tiles
    from the row count), the self-replaced uncond target rows agree to the fp32 engine's tolerance; behind the exit the taps hold the surviving rows"""
    from etainv import _capi
    from etainv.engine import AttnControl
    n = 2
    e = engines(torch.float32, 16)
    x, ctx = _ptp_inputs(n)
    eq, ca = torch.ones(n, 77).cuda(), torch.ones(n, 77).cuda()
    eq[:, 2] = 2.0
    names = e.tap_names()
    for self_on, exit_block, last_full in ((True, 12, "up_blocks.2.attentions.2"), (False, 9, "up_blocks.1.attentions.2")):
        mk = lambda first, ex: AttnControl(mode=_capi.ATTN_PTP, n_img=n, store_maps=True, equalizer=eq, cross_alpha=ca, self_replace_active=self_on,
                                           self_max_tokens=64, first_row=first, src_exit_block=ex)
        e.maps_reset()
        full, taps4 = tapped_forward(e, x, 481, ctx, mk(0, 0))
        e.maps_reset()
        three, taps3 = tapped_forward(e, torch.cat([x[n:], x[:n]]), 481, ctx[n:].contiguous(), mk(n, 0))      # rows [u_t, c_s, c_t]
        assert torch.equal(three[n:], full[2 * n:])
        for name in names:
            assert taps3[name].shape[0] == 3 * n and taps4[name].shape[0] == 4 * n, name
            assert torch.equal(taps3[name][n:], taps4[name][2 * n:]), name
            err = float((taps3[name][:n].double() - taps4[name][n:2 * n].double()).norm() / taps4[name][n:2 * n].double().norm())
            assert err < 1e-5, (name, err)
        e.maps_reset()
        ctx_x = torch.cat([ctx[n:2 * n], ctx[3 * n:], ctx[2 * n:3 * n]]).contiguous()                        # rows [u_t, c_t, c_s]
        ex, taps_x = tapped_forward(e, torch.cat([x[n:], x[n:], x[:n]]), 481, ctx_x, mk(n, exit_block))
        assert torch.equal(ex[:n], three[:n]) and torch.equal(ex[n:2 * n], three[2 * n:])
        cut = names.index(last_full)
        for k, name in enumerate(names):
            a, b = taps_x[name], taps3[name]
            assert e.tap_rows(name) == a.shape[0] == (3 * n if k <= cut else 2 * n), (name, a.shape)
            assert torch.equal(a[:n], b[:n]) and torch.equal(a[n:2 * n], b[2 * n:]), name                    # u_t, c_t: the surviving rows
            if k <= cut:
                assert torch.equal(a[2 * n:], b[n:2 * n]), name                                              # c_s, until it leaves
