"""Whole-UNet parity on MI355X: the native executor (C ABI etainv_unet_forward) vs the CPU oracle's fp32 UNet
restatement on identical synthetic SD1.x weights, inputs and attention controls."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


from tests.oracle_cache import oracle_leg, oracle_unet  # noqa: E402


@pytest.fixture(scope="module")
def engines():
    from etainv.engine import Engine
    made = {}

    def get(dtype, L):
        key = (dtype, L)
        if key not in made:
            e = Engine(dtype=dtype, max_unet_batch=8, latent_size=L, max_img=2)
            e.load_synthetic(0)
            made[key] = e
        return made[key]
    yield get
    for e in made.values():
        e.close()


def relerr(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def test_weight_names_match_oracle(engines):
    from oracle.unet import UNet2DConditionModel
    e = engines(torch.float16, 16)
    specs = dict(e.weight_specs())
    with torch.device("meta"):                       # names and shapes only (the values are compared below, tensor by tensor)
        sd = UNet2DConditionModel().state_dict()
    assert set(specs) == set(sd.keys())
    for k, v in sd.items():
        assert tuple(v.shape) == specs[k], k
    from etainv.weights import synthetic_tensor
    from oracle.unet import synthetic_tensor as oracle_syn
    for name in ("conv_in.weight", "mid_block.attentions.0.transformer_blocks.0.ff.net.0.proj.bias", "up_blocks.3.resnets.2.conv2.weight"):
        assert torch.equal(synthetic_tensor(name, specs[name], 0), oracle_syn(name, specs[name], 0))


FWD_CASES = [(16, 2, 500), (32, 4, 981), (16, 4, 0)]


def _fwd_inputs(L, rows):
    g = torch.Generator().manual_seed(L * 100 + rows)
    return torch.randn(rows // 2, 4, L, L, generator=g), torch.randn(rows, 77, 768, generator=g)


@oracle_leg(cases=FWD_CASES)
def leg_unet_forward(L, rows, t):
    latent, ctx = _fwd_inputs(L, rows)
    return {"ref": oracle_unet()(torch.cat([latent] * 2), torch.tensor(t), encoder_hidden_states=ctx)["sample"]}


@oracle_leg()
def leg_unet_bench_shape():
    g = torch.Generator().manual_seed(1)
    x1, c1 = torch.randn(1, 4, 64, 64, generator=g), torch.randn(1, 77, 768, generator=g)
    return {"ref": oracle_unet()(x1, 500, encoder_hidden_states=c1)["sample"][0]}


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 4e-3), (torch.bfloat16, 3e-2)])
@pytest.mark.parametrize("L,rows,t", FWD_CASES)
def test_unet_forward_vs_oracle(engines, dtype, tol, L, rows, t):
    latent, ctx = _fwd_inputs(L, rows)
    ref = leg_unet_forward(L, rows, t)["ref"]
    e = engines(dtype, L)
    out = e.unet(latent.cuda(), t, ctx.cuda())
    torch.cuda.synchronize()
    err = relerr(out.cpu(), ref)
    print(f"L={L} rows={rows} t={t} {dtype}: rel L2 {err:.2e}, max abs {float((out.cpu() - ref).abs().max()):.2e}")
    assert err < tol


def test_unet_bench_shape_class_vs_oracle():
    """L = 64 with 16 UNet rows: the tile dispatch of the bench configuration (256 x 160 / 256 x 128 persistent ring kernels,
    several tiles per block, two-slot kernels for the fused-upsample convs), which small-L tests never reach.  The same sample in
    every row, so one CPU-oracle forward checks all rows; rows must also agree bit for bit with each other."""
    from etainv.engine import Engine
    e = Engine(dtype=torch.float16, max_unet_batch=16, latent_size=64, max_img=4)
    e.load_synthetic(0)
    g = torch.Generator().manual_seed(1)
    x1, c1 = torch.randn(1, 4, 64, 64, generator=g), torch.randn(1, 77, 768, generator=g)
    ref = leg_unet_bench_shape()["ref"]
    for rows in (1, 4, 16):
        out = torch.empty(rows, 4, 64, 64, device="cuda")
        e.unet(x1.repeat(rows, 1, 1, 1).cuda().contiguous(), 500, c1.repeat(rows, 1, 1).cuda().contiguous(), None, out=out)
        torch.cuda.synchronize()
        assert all(torch.equal(out[0], out[i]) for i in range(rows))
        assert relerr(out[0].cpu(), ref) < 3e-3, rows
    e.close()


@pytest.mark.parametrize("switch", ["ETAINV_LN_UNFUSED", "ETAINV_GN_UNFUSED"])
def test_unet_norm_fusion_switches_agree(monkeypatch, switch):
    """the A/B switches of the norm fusions (LayerNorm folded into the GEMMs around it, GroupNorm statistics from the producer's epilogue) change
    where the arithmetic happens, not the result: same weights and inputs, L = 32 (both
    fused paths and their fallbacks at the 4 x 4 level), against the default engine"""
    from etainv.engine import Engine
    g = torch.Generator().manual_seed(5)
    # 16 UNet rows: enough tiles that the level-0 convs run unsplit (a split-K producer emits no statistics, and then nothing is fused behind it)
    x, ctx = torch.randn(8, 4, 32, 32, generator=g).cuda(), torch.randn(16, 77, 768, generator=g).cuda()
    outs = []
    for on in (False, True):
        if on:
            monkeypatch.setenv(switch, "1")
        e = Engine(dtype=torch.float16, max_unet_batch=16, latent_size=32, max_img=4)
        e.load_synthetic(0)
        outs.append(e.unet(x, 500, ctx).float().cpu())
        torch.cuda.synchronize()
        e.close()
    err = relerr(outs[1], outs[0])
    print(f"{switch}: rel L2 {err:.2e}")
    assert 0 < err < 2e-3


def test_context_cache_reuses_projections_and_tracks_changes(engines):
    """etainv_engine_cache_context: a second call with the same context tensor reuses the cross-attention K / V projections (same output bit
    for bit); a different tensor, a different row count, or switching the cache off and on recomputes them"""
    e = engines(torch.float16, 16)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 4, 16, 16, generator=g).cuda()
    c1, c2 = torch.randn(4, 77, 768, generator=g).cuda(), torch.randn(4, 77, 768, generator=g).cuda()
    ref1, ref2 = e.unet(x, 300, c1).clone(), e.unet(x, 300, c2).clone()
    assert not torch.equal(ref1, ref2)
    e.cache_context(True)
    try:
        assert torch.equal(e.unet(x, 300, c1), ref1)
        assert torch.equal(e.unet(x, 300, c1), ref1)          # projections reused
        assert torch.equal(e.unet(x, 300, c2), ref2)          # another tensor: recomputed
        assert torch.equal(e.unet(x[:1], 300, c2[:2]), e.unet(x[:1], 300, c2[:2].clone()))   # fewer rows, same base pointer: recomputed
        c2.copy_(c1)                                          # contents changed behind the engine's back: the caller's promise is broken,
        e.cache_context(True)                                 # re-arming the cache is what a loop start does
        assert torch.equal(e.unet(x, 300, c2), ref1)
    finally:
        e.cache_context(False)
    assert torch.equal(e.unet(x, 300, c1), ref1)


def test_context_cache_generation_and_error_paths(engines):
    """ADVICE r2 / VERDICT r2 item 10: (i) a context rewritten IN PLACE is picked up when the caller bumps the generation
    (etainv_engine_context_generation) -- and, documented, NOT picked up otherwise; (ii) `with engine.cached_context()` switches the cache off on
    an exception; (iii) a forward that fails validation does not leave a cache entry behind."""
    from etainv import _capi
    e = engines(torch.float16, 16)
    g = torch.Generator().manual_seed(19)
    x = torch.randn(2, 4, 16, 16, generator=g).cuda()
    c1, c2 = torch.randn(4, 77, 768, generator=g).cuda(), torch.randn(4, 77, 768, generator=g).cuda()
    ref1, ref2 = e.unet(x, 300, c1).clone(), e.unet(x, 300, c2).clone()
    buf = c1.clone()
    with e.cached_context():
        assert torch.equal(e.unet(x, 300, buf), ref1)
        buf.copy_(c2)                                                       # same pointer, rows, dtype -- new contents
        assert torch.equal(e.unet(x, 300, buf), ref1)                       # the promise "unchanged" was broken: stale K / V (by contract)
        _capi.check(e.lib.etainv_engine_context_generation(e.h, 1 << 40))   # the caller says so: recomputed
        assert torch.equal(e.unet(x, 300, buf), ref2)
    with pytest.raises(RuntimeError):
        with e.cached_context():
            e.unet(x, 300, buf)
            raise RuntimeError("loop body failed")
    buf.copy_(c1)                                                           # the cache must be off now: every call projects what it is given
    assert torch.equal(e.unet(x, 300, buf), ref1)
    with e.cached_context():
        big = torch.randn(16, 77, 768, generator=g).cuda()                  # 16 rows > max_unet_batch = 8: the call fails before any launch
        with pytest.raises(_capi.EtainvError):
            e.unet(x, 300, big)
        assert torch.equal(e.unet(x, 300, buf), ref1)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("mode", ["plain", "ptp", "masa"])
def test_context_independent_prefix_is_shared_not_changed(engines, dtype, mode):
    """A CFG call carries every latent twice (uncond / cond rows): conv_in, the first residual block and the first transformer block up to its
    cross-attention do not read the context and run on half the rows (engine.cpp, etainv_unet_forward).  The result must equal the unshared execution
    (ETAINV_NO_PREFIX_SHARE=1) bit for bit -- with the attention controls of the backward pass too -- and rows with DIFFERENT timesteps must not
    be shared."""
    import os
    from etainv import _capi
    from etainv.engine import AttnControl
    e = engines(dtype, 16)
    g = torch.Generator().manual_seed(21)
    n_img = 2
    x = torch.randn(2 * n_img, 4, 16, 16, generator=g).cuda()              # [src.., tgt..]
    ctx = torch.randn(4 * n_img, 77, 768, generator=g).cuda()              # [u_s.., u_t.., c_s.., c_t..]
    ca = torch.ones(n_img, 77).cuda()
    mapper = torch.arange(77, dtype=torch.int32).repeat(n_img, 1).cuda()
    al = torch.ones(n_img, 77).cuda()

    def ctrl():
        if mode == "ptp":
            return AttnControl(mode=_capi.ATTN_PTP, n_img=n_img, store_maps=False, mapper=mapper, alphas=al, cross_alpha=ca, self_replace_active=True,
                               self_max_tokens=64)
        if mode == "masa":
            return AttnControl(mode=_capi.ATTN_MASA, n_img=n_img, masa_active=True, masa_first_block=10)
        return None
    # (split-K picks its part count from the tile count, i.e. from the row count: pinned off for the bit-for-bit comparison, on for the close one)
    os.environ["ETAINV_NO_SPLITK"] = "1"
    try:
        shared = e.unet(x, 481, ctx, ctrl()).clone()
        os.environ["ETAINV_NO_PREFIX_SHARE"] = "1"
        full = e.unet(x, 481, ctx, ctrl()).clone()
    finally:
        os.environ.pop("ETAINV_NO_PREFIX_SHARE", None)
        del os.environ["ETAINV_NO_SPLITK"]
    assert torch.equal(shared, full)
    assert relerr(e.unet(x, 481, ctx, ctrl()), full) < (1e-5 if dtype == torch.float32 else 2e-3 if dtype == torch.float16 else 1.5e-2)
    assert not torch.equal(shared[:2 * n_img], shared[2 * n_img:])           # the halves differ (different contexts)
    if mode == "plain":                                                      # per-row timesteps that differ between the halves: no sharing, still right
        t = [481] * (2 * n_img) + [301] * (2 * n_img)
        a = e.unet(x, t, ctx)
        b = torch.cat([e.unet(x, 481, ctx[:2 * n_img].contiguous()), e.unet(x, 301, ctx[2 * n_img:].contiguous())])
        assert relerr(a, b) < (1e-5 if dtype == torch.float32 else 2e-3 if dtype == torch.float16 else 1.5e-2)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_three_row_layout_equals_the_four_row_call(engines, dtype):
    """etainv_attn_ctrl.first_row = n_img: a prompt-to-prompt call WITHOUT its uncond source rows (rows [u_t, c_s, c_t] over latents [tgt, src]; the
    backward steps with eta == 0, etainv/pipeline.py) gives the same u_t / c_s / c_t outputs as the full [u_s, u_t, c_s, c_t] call -- with the cross
    edit, the self-replace remap and the map store active -- and the same stored maps."""
    from etainv import _capi
    from etainv.engine import AttnControl
    e = engines(dtype, 16)
    n = 2
    g = torch.Generator().manual_seed(33)
    x = torch.randn(2 * n, 4, 16, 16, generator=g).cuda()                       # [src.., tgt..]
    ctx = torch.randn(4 * n, 77, 768, generator=g).cuda()                       # [u_s, u_t, c_s, c_t]
    mapper = torch.arange(77, dtype=torch.int32).repeat(n, 1)
    mapper[:, 2] = -1
    al = torch.ones(n, 77)
    al[:, 2] = 0
    eq = torch.ones(n, 77)
    eq[:, 2] = 2.0
    mapper, al, eq, ca = mapper.cuda(), al.cuda(), eq.cuda(), torch.ones(n, 77).cuda()
    tokens = torch.arange(1, 5, dtype=torch.int32).repeat(n, 1).cuda()
    mk = lambda first: AttnControl(mode=_capi.ATTN_PTP, n_img=n, store_maps=True, mapper=mapper, alphas=al, equalizer=eq, cross_alpha=ca,
                                   self_replace_active=True, self_max_tokens=64, first_row=first)
    os_env = __import__("os").environ
    os_env["ETAINV_NO_SPLITK"] = "1"                                             # (split-K part counts follow the row count: pinned for bit equality)
    try:
        e.maps_reset()
        full = e.unet(x, 481, ctx, mk(0)).clone()
        maps_full = e.word_maps(n, tokens, 1, torch.empty(n, 4, 16, 16, device="cuda")).clone()
        e.maps_reset()
        three = e.unet(torch.cat([x[n:], x[:n]]), 481, ctx[n:].contiguous(), mk(n)).clone()
        maps_three = e.word_maps(n, tokens, 1, torch.empty(n, 4, 16, 16, device="cuda")).clone()
    finally:
        del os_env["ETAINV_NO_SPLITK"]
    tol = 1e-5 if dtype == torch.float32 else 2e-3
    assert relerr(three, full[n:]) < tol and relerr(maps_three, maps_full) < tol
    if dtype == torch.float32:                                                   # (the 16-bit GEMMs pick their tile shape from the row count; the fp32 kernel does not)
        assert torch.equal(three[n:], full[2 * n:])                              # the cond rows do not depend on which uncond rows ride along
    # src_exit_block: rows [u_t, c_t, c_s], no cross edit; the cond source rows leave after block 12 (self-replace still active: the (L/2)^2-token
    # self-attentions read their Q, K) or after block 9 (store only) -- the u_t / c_t outputs and the stored maps equal the full call's
    for self_on, exit_block in ((True, 12), (False, 9)):
        mk2 = lambda first, ex: AttnControl(mode=_capi.ATTN_PTP, n_img=n, store_maps=True, equalizer=eq, cross_alpha=ca, self_replace_active=self_on,
                                            self_max_tokens=64, first_row=first, src_exit_block=ex)
        e.maps_reset()
        full2 = e.unet(x, 481, ctx, mk2(0, 0)).clone()
        maps_full2 = e.word_maps(n, tokens, 1, torch.empty(n, 4, 16, 16, device="cuda")).clone()
        e.maps_reset()
        ctx_x = torch.cat([ctx[n:2 * n], ctx[3 * n:], ctx[2 * n:3 * n]]).contiguous()                  # [u_t, c_t, c_s]
        ex = e.unet(torch.cat([x[n:], x[n:], x[:n]]), 481, ctx_x, mk2(n, exit_block)).clone()
        maps_ex = e.word_maps(n, tokens, 1, torch.empty(n, 4, 16, 16, device="cuda")).clone()
        assert relerr(ex[:n], full2[n:2 * n]) < tol and relerr(ex[n:2 * n], full2[3 * n:]) < tol and relerr(maps_ex, maps_full2) < tol
    # the same context tensor under the context cache, block-9 exit FIRST: the later block-12 exit must find K / V of all rows in the cache
    ctx_x = torch.cat([ctx[n:2 * n], ctx[3 * n:], ctx[2 * n:3 * n]]).contiguous()
    mk3 = lambda self_on, ex: AttnControl(mode=_capi.ATTN_PTP, n_img=n, store_maps=True, equalizer=eq, cross_alpha=ca, self_replace_active=self_on,
                                          self_max_tokens=64, first_row=n, src_exit_block=ex)
    lat_x = torch.cat([x[n:], x[n:], x[:n]])
    want = e.unet(lat_x, 481, ctx_x, mk3(True, 12)).clone()
    e.unet(lat_x, 481, torch.randn(3 * n, 77, 768, generator=g).cuda(), mk3(True, 12))       # (another context: the K / V buffers now hold foreign rows)
    with e.cached_context():
        e.unet(lat_x, 481, ctx_x, mk3(False, 9))
        got = e.unet(lat_x, 481, ctx_x, mk3(True, 12)).clone()
    assert torch.equal(got[:2 * n], want[:2 * n])
    with pytest.raises(_capi.EtainvError):                                       # an exit in front of the last self-replace layer would starve it
        e.unet(torch.cat([x[n:], x[n:], x[:n]]), 481, ctx_x, mk2(n, 9) if False else AttnControl(
            mode=_capi.ATTN_PTP, n_img=n, store_maps=True, cross_alpha=ca, self_replace_active=True, self_max_tokens=64, first_row=n, src_exit_block=9))
    with pytest.raises(_capi.EtainvError):                                       # MasaCtrl couples u_t to u_s: no three-row form
        e.unet(torch.cat([x[n:], x[:n]]), 481, ctx[n:].contiguous(), AttnControl(mode=_capi.ATTN_MASA, n_img=n, masa_active=True, first_row=n))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_head_major_qkv_planes_equal_the_row_major_layout(monkeypatch, dtype):
    """Head-major QKV planes (default; ETAINV_QKV_HM=0 = row-major): the fused QKV projection stores three head-major planes and the head_dim 40 / 80 self-attention kernel reads 64-key tiles as
    contiguous blocks (csrc/igemm.hip role 4, csrc/attention.hip hm_rows).  Only the layout of an intermediate changes: outputs must be BIT-identical --
    plain rows, the shared prefix of a CFG call, the MasaCtrl K / V remap, the prompt-to-prompt self-replace (Q, K of the source rows) with the
    three-row layout and the early exit.  The counter proves the path ran (L = 64, 4+ rows: the 256 x 160 ring takes the QKV GEMMs of both levels)."""
    from etainv import _capi
    from etainv.engine import AttnControl, Engine
    L, rows = 64, 8
    res = []
    for hm in (True, False):
        monkeypatch.setenv("ETAINV_QKV_HM", "1" if hm else "0")          # (read at engine creation; on by default)
        e = Engine(dtype=dtype, max_unet_batch=rows, latent_size=L, max_img=2)
        e.load_synthetic(0)
        g = torch.Generator().manual_seed(21)
        x2 = torch.randn(2, 4, L, L, generator=g).cuda()
        x4 = torch.randn(4, 4, L, L, generator=g).cuda()
        ctx = torch.randn(rows, 77, 768, generator=g).cuda()
        outs = [e.unet(x4, [500] * 4 + [480] * 4, ctx).clone(),                                      # 8 different rows (pairs at different timesteps: no shared prefix)
                e.unet(x4, 700, ctx).clone(),                                                        # CFG call: rows r and r + 4 share the prefix
                e.unet(x4, 300, ctx, AttnControl(mode=_capi.ATTN_MASA, n_img=2, masa_active=True, masa_first_block=10)).clone()]
        ones = torch.ones(2, 77, device="cuda")
        ptp = lambda first, ex: AttnControl(mode=_capi.ATTN_PTP, n_img=2, store_maps=True, equalizer=ones, cross_alpha=ones, self_replace_active=True,
                                            self_max_tokens=(L // 2) ** 2, first_row=first, src_exit_block=ex)
        e.maps_reset()
        outs.append(e.unet(x4, 481, ctx, ptp(0, 0)).clone())                                         # [u_s, u_t, c_s, c_t] x 2, self-replace at the 32^2 level
        ctx3 = torch.cat([ctx[2:4], ctx[6:8], ctx[4:6]]).contiguous()                                # rows [u_t, c_t, c_s] over latents [tgt, tgt, src]:
        outs.append(e.unet(torch.cat([x4[2:], x4[2:], x4[:2]]), 481, ctx3, ptp(2, 12))[:4].clone())  # the cond source rows leave after block 12
        torch.cuda.synchronize()
        res.append((outs, e.qkv_head_major_launches))
        e.close()
    (a, n_hm), (b, n_rm) = res
    assert n_rm == 0 and n_hm >= 5 * 4, (n_hm, n_rm)                      # (5 transformer blocks at each of the two levels per call, some calls on half the rows)
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.isfinite(u).all() and torch.equal(u, v), f"call {i}: head-major planes changed the result"
