"""Per-op parity of the kernels that the suite otherwise reaches only through a whole loop or a whole UNet call: csrc/step_kernels.hip, csrc/maps.hip and
the small kernels of csrc/misc.hip, with the two GEMM forms only the UNet launches (fp32 time projections read by the convs as a strided row; per-image
weights behind a folded GroupNorm).  Every reference is plain torch / numpy in float64 (the GEMM-class ones in fp32) of the inputs AFTER their rounding to the
io type.  Bounds: fp32 io 1e-5 (losses 2e-4); 16-bit io of an elementwise kernel one ulp of the type (one rounding of an fp32 result); GEMM-class results
the TOL table of tests/test_kernels_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import step_ref
from tests.test_aux_kernels_gpu import assert_guard, guarded_flat
from tests.test_kernels_gpu import TOL, capi, pack_geglu, relerr, rnd  # noqa: F401  (capi: fixture)

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
DTYPES3 = [torch.float32, torch.float16, torch.bfloat16]
ULP = {torch.float32: 1e-5, torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}     # rtol = atol of an elementwise kernel per io type
NAN = float("nan")


def close64(out, ref, tol, equal_nan=False):
    torch.testing.assert_close(out.detach().cpu().double(), ref.detach().cpu().double(), rtol=tol, atol=tol, equal_nan=equal_nan)


def bits(t):
    """the tensor's bit patterns (so that -0 / +0 and NaN payloads count)"""
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def round_once(x64, dtype):
    """float64 -> a 16-bit type with ONE rounding to nearest even (torch converts a double through fp32: two roundings)"""
    if dtype == torch.float16:
        return torch.from_numpy(x64.cpu().numpy().astype(np.float16))
    b64 = x64.cpu().contiguous().view(torch.int64)                       # bf16 keeps 7 of the 52 fraction bits and has fp32's exponent range
    b64 = (b64 + ((b64 >> 45) & 1) + (2 ** 44 - 1)) & ~(2 ** 45 - 1)
    return b64.view(torch.float64).to(torch.bfloat16)


def urand(*shape, seed, lo=0.0, hi=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * (hi - lo) + lo).to(dtype).cuda()


# ----------------------------------------------------------------------------------------- step kernels
N_LOOP = 2 * 2048 * 256 + 77      # the grid is capped at 2048 blocks of 256 threads: two full passes of the grid-stride loop and a ragged third


def test_grid_stride_loop(capi):
    """cfg_combine, ddim_step, lincomb3 beyond the 2048-block cap (the loops run B = 32 at n = 524288 = the cap exactly; any larger batch loops)"""
    from oracle import schedule as sch
    lib, n, s = capi.load(), N_LOOP, capi.stream_ptr()
    x, y, z = rnd(n, seed=1), rnd(n, seed=2), rnd(n, seed=3)
    x64, y64, z64 = x.cpu().double(), y.cpu().double(), z.cpu().double()
    a_from, a_to = sch.ddim_inverse_coeffs(sch.alphas_cumprod(), 500, 50)
    cases = {
        "cfg_combine": (lambda o: lib.etainv_cfg_combine(capi.ptr(x), capi.ptr(y), 7.5, capi.ptr(o), n, capi.F32, s), x64 + 7.5 * (y64 - x64)),
        "ddim_step": (lambda o: lib.etainv_ddim_step(capi.ptr(x), capi.ptr(y), a_from, a_to, capi.ptr(o), n, capi.F32, s), sch.ddim_step(x64, y64, a_from, a_to)),
        "lincomb3": (lambda o: lib.etainv_lincomb3(capi.ptr(x), 1.3, capi.ptr(y), -0.7, None, 0.45, capi.ptr(o), n, capi.F32, s), 1.3 * x64 - 0.7 * y64),
        "lincomb3_z": (lambda o: lib.etainv_lincomb3(capi.ptr(x), 1.3, capi.ptr(y), -0.7, capi.ptr(z), 0.45, capi.ptr(o), n, capi.F32, s),
                       1.3 * x64 - 0.7 * y64 + float(np.float32(0.45)) * z64),
    }
    for name, (launch, ref) in cases.items():
        out = guarded_flat(n, torch.float32, 256)
        capi.check(launch(out))
        assert_guard(out, n)
        close64(out[:n], ref, 1e-5)
        close64(out[n - 77:n], ref[n - 77:], 1e-5)                       # the ragged third pass
    out = guarded_flat(16, torch.float32, 16)                            # n = 0 is a no-op
    capi.check(lib.etainv_lincomb3(capi.ptr(x), 1.3, capi.ptr(y), -0.7, capi.ptr(z), 0.45, capi.ptr(out), 0, capi.F32, s))
    torch.cuda.synchronize()
    assert torch.isnan(out[:16]).all()


@pytest.mark.parametrize("dtype", DTYPES3)
@pytest.mark.parametrize("rows", [4, 3])          # rows * chw = 2304 = 9 blocks exactly / 1728: a ragged last block
@pytest.mark.parametrize("case", ["eta0", "noise", "mask"])
def test_ddim_eta_step_vs_oracle(capi, dtype, rows, case):
    """etainv_ddim_eta_step against oracle.schedule.ddim_eta_step: eta = 0 without mask or noise (the form the pipeline launches), eta = 0.4 with the noise
    shared by all rows, and with two masks for the rows (row r reads mask r % 2).  t = 0 < 1000 / S: a_p = ac[0] and var = 0 are what the host passes."""
    from oracle import schedule as sch
    lib, ac, S, c, h = capi.load(), sch.alphas_cumprod(), 50, 4, 12
    x, eps = rnd(rows, c, h, h, seed=1, dtype=dtype), rnd(rows, c, h, h, seed=2, dtype=dtype)
    noise = None if case == "eta0" else rnd(c, h, h, seed=3, dtype=dtype)
    mask = urand(2, h, h, seed=4, dtype=dtype) if case == "mask" else None
    eta = 0.0 if case == "eta0" else 0.4
    eta_ref = float(np.float32(eta))
    if mask is not None:
        eta_ref = eta_ref * torch.stack([mask[r % 2] for r in range(rows)]).cpu().double()[:, None]
    n = rows * c * h * h
    for t in (0, 20, 500, 980):
        p = t - 1000 // S
        a_t, a_p, var = float(ac[t]), float(ac[p]) if p >= 0 else float(ac[0]), sch.variance(ac, t, S)
        if p < 0:
            assert a_p == a_t == float(ac[0]) and var == 0.0
        out = guarded_flat(n, dtype, 256)
        capi.check(lib.etainv_ddim_eta_step(capi.ptr(x), capi.ptr(eps), eta, capi.ptr(mask), 2 if mask is not None else 0, capi.ptr(noise), a_t, a_p, var,
                                            rows, c, h * h, capi.ptr(out), capi.dtype_code(dtype), capi.stream_ptr()))
        assert_guard(out, n)
        ref = sch.ddim_eta_step(x.cpu().double(), eps.cpu().double(), ac, t, S, eta_ref, noise=None if noise is None else noise.cpu().double())
        close64(out[:n].view(rows, c, h, h), ref, ULP[dtype])


def _eta_inputs(n_img, c, side, n_cand, dtype, winners, eta, t, S, ac):
    """inputs of the fused backward step with the winner PLANTED: x_prev[i] = mean_i + std * noise[winners[i]] (then rounded to the io type, like every input)"""
    from oracle import schedule as sch
    x, eps_all = rnd(2 * n_img, c, side, side, seed=11, dtype=dtype), rnd(4 * n_img, c, side, side, seed=12, dtype=dtype)
    noise = rnd(n_cand, c, side, side, seed=13, dtype=dtype)
    x64, e64, z64 = x.cpu().double(), eps_all.cpu().double(), noise.cpu().double()
    std = eta * sch.variance(ac, t, S) ** 0.5
    xp = []
    for i in range(n_img):
        eps_s = e64[i] + step_ref.G * (e64[2 * n_img + i] - e64[i])
        xp.append(sch.ddim_eta_step(x64[i], eps_s, ac, t, S, eta, noise=None) + std * z64[winners[i]])
    x_prev = torch.stack(xp).to(dtype).cuda()
    mask, dmap = urand(n_img, side, side, seed=14, dtype=dtype), urand(n_img, side, side, seed=15, dtype=dtype)
    return x, eps_all, x_prev, noise, mask, dmap


def _eta_launch(capi, x, eps_all, x_prev, noise, eta, mask, thres, use_mask, ac, t, S, n_img, tdir=0.0, dmap=None):
    from oracle import schedule as sch
    lib = capi.load()
    p = t - 1000 // S
    c, hw, n_cand = x.shape[1], x.shape[2] * x.shape[3], noise.shape[0]
    n = x.numel()
    out_x, out_eps = guarded_flat(n, x.dtype, 256), guarded_flat(n, x.dtype, 256)
    best = torch.full((n_img + 4,), -7, dtype=torch.int32, device="cuda")
    losses = guarded_flat(n_img * n_cand, torch.float32, 16)
    scratch = torch.full((n_img * 16 * 64,), NAN, dtype=torch.float32, device="cuda")
    capi.check(lib.etainv_eta_backward_step_ex(capi.ptr(x), capi.ptr(eps_all), step_ref.G, capi.ptr(x_prev), capi.ptr(noise), n_cand, eta, capi.ptr(mask), thres,
                                               use_mask, float(ac[t]), float(ac[p]) if p >= 0 else float(ac[0]), sch.variance(ac, t, S), n_img, c, hw,
                                               capi.ptr(out_x), capi.ptr(out_eps), capi.ptr(best), capi.ptr(losses), capi.ptr(scratch),
                                               capi.dtype_code(x.dtype), tdir, capi.ptr(dmap), capi.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(best[n_img:].cpu(), torch.full((4,), -7, dtype=torch.int32)), "best_idx written behind n_img"
    return out_x, out_eps, best[:n_img].cpu().long(), losses


# |fp32 torch restatement - float64| of the planted winner's loss, the largest over the cases of the test below, per io type (measured on the CPU)
WINNER_LOSS_F32_ERR = {torch.float32: 3.8e-11, torch.float16: 3.7e-9, torch.bfloat16: 4.1e-8}


@pytest.mark.parametrize("dtype", DTYPES3)
@pytest.mark.parametrize("n_cand", [1, 10, 16])
@pytest.mark.parametrize("n_img,c,side", [(1, 4, 2), (3, 4, 12), (2, 4, 24)])     # chw = 16 (< the 64 loss blocks), 576 = 64 * 9, 2304 = 64 * 36; hw = 4, 144, 576
def test_eta_backward_step_vs_restatement(capi, dtype, n_img, c, side, n_cand):
    """etainv_eta_backward_step_ex against tests/step_ref.py for use_mask 0 / 1 / 2, target_dirinv off / on, dirinv_map absent / present: both roles of
    out_x, out_eps, best and losses[img][j].  The winner of every image is planted (another one per image), so no choice rests on a close call."""
    from oracle import schedule as sch
    ac, t, S, eta, thres = sch.alphas_cumprod(), 500, 50, 0.4, 0.2
    winners = [(3 + 5 * i) % n_cand for i in range(n_img)]
    x, eps_all, x_prev, noise, mask, dmap = _eta_inputs(n_img, c, side, n_cand, dtype, winners, float(np.float32(eta)), t, S, ac)
    n, tol, worst_winner = x.numel(), ULP[dtype], 0.0
    for use_mask in (0, 1, 2):
        for tdir, dm in ((0.0, None), (0.0, dmap), (0.6, None), (0.6, dmap)):
            if tdir and not use_mask:
                continue                      # refused: test_eta_backward_step_refusals
            ox, oe, best, losses = _eta_launch(capi, x, eps_all, x_prev, noise, eta, mask, thres, use_mask, ac, t, S, n_img, tdir, dm)
            rx, re, rbest, rloss = step_ref.eta_backward_step_ref(x, eps_all, step_ref.G, x_prev, noise, float(np.float32(eta)), mask, thres, use_mask, ac, t, S,
                                                                         float(np.float32(tdir)), dm)
            label = f"use_mask={use_mask} tdir={tdir} dirinv_map={dm is not None}"
            assert rbest.tolist() == winners, label
            if n_cand > 1:                    # on the reference alone: the two smallest losses are far apart
                two = rloss.sort(dim=1).values[:, :2]
                assert bool(((two[:, 1] - two[:, 0]) > 1e-3 * two[:, 1]).all()), label
            assert best.tolist() == rbest.tolist(), label
            assert_guard(ox, n)
            assert_guard(oe, n)
            assert_guard(losses, n_img * n_cand)
            close64(ox[:n].view_as(x), rx, tol)
            close64(oe[:n].view_as(x), re, tol)
            if use_mask == 0:
                assert torch.equal(ox[:n].view_as(x)[:n_img], x_prev), label + ": the source rows are the stored latents, bit for bit"
            # losses[img][j]: rtol 2e-4, which every loss but the planted winner's meets.  That one is no signal but the residue of rounding x_prev to
            # the io type (1e-14 in fp32 io), which rtol cannot express: the same arithmetic in fp32 torch (step_ref.eta_backward_step_ref with
            # dtype = float32, over all the cases of this test) is off float64 by at most WINNER_LOSS_F32_ERR there; the winner gets twice that as atol.
            got = losses[:n_img * n_cand].view(n_img, n_cand).cpu().double()
            atol = torch.zeros_like(rloss)
            for i, j in enumerate(winners):
                atol[i, j] = 2 * WINNER_LOSS_F32_ERR[dtype]
                worst_winner = max(worst_winner, abs(float(got[i, j] - rloss[i, j])))
            assert bool(((got - rloss).abs() <= 2e-4 * rloss + atol).all()), (label, got, rloss)
    print(f"eta_backward_step {dtype} ({n_img}, {c}, {side * side}) n_cand={n_cand}: planted winner's loss off by at most {worst_winner:.3e} "
          f"(bound {2 * WINNER_LOSS_F32_ERR[dtype]:.3e})")


@pytest.mark.parametrize("case", ["tie", "nan_above_winner", "two_nans"])
def test_eta_backward_step_argmin_contract(capi, case):
    """"first NaN wins, else first minimum" (torch.argmin of the reference losses): two identical planted candidates -> the lower index; a candidate with one
    NaN element above the planted winner -> the NaN candidate; two NaN candidates -> the lower one.  NaN is a value here, not a fault."""
    from oracle import schedule as sch
    ac, t, S, eta, n_img, c, side, n_cand = sch.alphas_cumprod(), 500, 50, float(np.float32(0.4)), 3, 4, 12, 10
    x, eps_all, x_prev, noise, mask, _ = _eta_inputs(n_img, c, side, n_cand, torch.float32, [3, 3, 3], eta, t, S, ac)
    if case == "tie":
        noise[7] = noise[3]
        expect = 3
    elif case == "nan_above_winner":
        noise[6, 2, 5, 7] = NAN
        expect = 6
    else:
        noise[8, 0, 0, 0] = NAN
        noise[5, 3, 11, 11] = NAN
        expect = 5
    ox, oe, best, losses = _eta_launch(capi, x, eps_all, x_prev, noise, eta, mask, 0.2, 1, ac, t, S, n_img)
    rx, re, rbest, rloss = step_ref.eta_backward_step_ref(x, eps_all, step_ref.G, x_prev, noise, eta, mask, 0.2, 1, ac, t, S)
    assert rbest.tolist() == [int(torch.argmin(rloss[i])) for i in range(n_img)] == [expect] * n_img
    assert best.tolist() == rbest.tolist()
    got = losses[:n_img * n_cand].view(n_img, n_cand).cpu().double()
    assert torch.equal(torch.isnan(got), torch.isnan(rloss))
    if case == "tie":
        assert torch.equal(got[:, 3], got[:, 7])
    n = x.numel()
    close64(ox[:n].view_as(x), rx, 1e-5, equal_nan=True)       # the chosen candidate's NaN element reaches both rows; every other element is exact
    close64(oe[:n].view_as(x), re, 1e-5)


def test_eta_backward_step_refusals(capi):
    from oracle import schedule as sch
    ac = sch.alphas_cumprod()
    x, eps_all, x_prev, noise, mask, dmap = _eta_inputs(1, 4, 2, 2, torch.float32, [0], 0.4, 500, 50, ac)
    with pytest.raises(capi.EtainvError, match="target_dirinv"):
        _eta_launch(capi, x, eps_all, x_prev, noise, 0.4, mask, 0.2, 0, ac, 500, 50, 1, 0.6, dmap)
    with pytest.raises(capi.EtainvError, match="mask_map"):
        _eta_launch(capi, x, eps_all, x_prev, noise, 0.4, None, 0.2, 1, ac, 500, 50, 1)
    noise17 = rnd(17, 4, 2, 2, seed=1)
    with pytest.raises(capi.EtainvError, match="noise_sample_count"):
        _eta_launch(capi, x, eps_all, x_prev, noise17, 0.4, mask, 0.2, 1, ac, 500, 50, 1)


# ----------------------------------------------------------------------------------------- map consumers
N_CAP, HEADS, STEPS = 3, 8, 3
FROM_WHERE = {0b11111: ("up", "down"), 0b00011: ("down",), 0b11100: ("up",)}
_STORES = {}


STORE_SEED = {6: 107, 16: 116, 24: 125}


def map_store(res):
    """a store [5 layers][n_img_cap = 3][2 roles][8 heads][res^2][77], "sums over 3 steps" (host copy, device copy); images 0 and 1 are used, 2 is the spare.
    Every (image, role, token) has its own blob on a low floor, so that maps have a shape and LocalBlend's threshold cuts through them."""
    if res not in _STORES:
        g = torch.Generator().manual_seed(STORE_SEED[res])
        yy, xx = torch.meshgrid(torch.arange(res, dtype=torch.float32), torch.arange(res, dtype=torch.float32), indexing="ij")
        cy, cx = torch.rand(N_CAP, 2, 1, 1, 77, generator=g) * res, torch.rand(N_CAP, 2, 1, 1, 77, generator=g) * res
        blob = 0.05 + torch.exp(-((yy[None, None, :, :, None] - cy) ** 2 + (xx[None, None, :, :, None] - cx) ** 2) / (2 * (res / 4) ** 2))
        acc = torch.rand(5, N_CAP, 2, HEADS, res * res, 77, generator=g) ** 4 * float(STEPS) * blob.reshape(1, N_CAP, 2, 1, res * res, 77)
        _STORES[res] = (acc, acc.cuda())
    return _STORES[res]


def ref_word_map(acc, img, tok, res, L, row_sel, layer_mask):
    """oracle.ptp.attention_map on the float64 store of one image, the way tests/test_kernels_gpu.py uses it (num_prompts = 2: the backward-pass store)"""
    from oracle import ptp as optp
    st = optp.AttentionStore()
    st.cur_step = STEPS
    lay = [acc[l, img].double().reshape(2 * HEADS, res * res, 77) for l in range(5)]
    st.attention_store = {"down_cross": lay[:2], "up_cross": lay[2:], "mid_cross": [], "down_self": [], "mid_self": [], "up_self": []}
    return optp.attention_map(st, tok, res=res, from_where=FROM_WHERE[layer_mask], resize=L, num_prompts=2, select=row_sel)[0]


def word_maps(capi, acc_d, res, L, tokens, row_sel, layer_mask, out=None, accumulate=0, scale=1.0):
    n_img, n_tok = tokens.shape
    buf = guarded_flat(n_img * n_tok * L * L, torch.float32, 1024)
    if out is not None:
        buf[:out.numel()] = out.flatten()
    capi.check(capi.load().etainv_op_word_maps_ex(capi.ptr(acc_d), 5, N_CAP, HEADS, res, L, n_img, capi.ptr(tokens), n_tok, STEPS, row_sel, layer_mask,
                                                  capi.ptr(buf), accumulate, scale, capi.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(buf[n_img * n_tok * L * L:].cpu(), torch.full((1024,), -777.0)), "the kernel wrote behind its output"
    return buf[:n_img * n_tok * L * L].view(n_img, n_tok, L, L).cpu()


@pytest.mark.parametrize("res,L", [(6, 24), (16, 16), (24, 96)])     # res^2 = 36 below one wave; res == L: no resampling; res^2 = 576 above the block size
@pytest.mark.parametrize("layer_mask", [0b11111, 0b00011, 0b11100])
@pytest.mark.parametrize("row_sel", [0, 1])
def test_word_maps_roles_layers_sizes(capi, res, L, layer_mask, row_sel):
    acc, acc_d = map_store(res)
    tokens = torch.tensor([[1, 2, 76], [3, 0, 4]], dtype=torch.int32).cuda()
    out = word_maps(capi, acc_d, res, L, tokens, row_sel, layer_mask)
    for img in range(2):
        for j in range(3):
            torch.testing.assert_close(out[img, j].double(), ref_word_map(acc, img, int(tokens[img, j]), res, L, row_sel, layer_mask), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("res,L", [(6, 24), (16, 16), (24, 96)])
def test_word_maps_single_token_accumulate_and_out_of_range(capi, res, L):
    acc, acc_d = map_store(res)
    ref = lambda img, tok, sel=1, lm=0b11111: ref_word_map(acc, img, tok, res, L, sel, lm)
    # n_tok = 1
    tokens = torch.tensor([[5], [9]], dtype=torch.int32).cuda()
    out = word_maps(capi, acc_d, res, L, tokens, 1, 0b11111)
    for img in range(2):
        torch.testing.assert_close(out[img, 0].double(), ref(img, int(tokens[img, 0])), rtol=1e-4, atol=1e-5)
    # accumulate = 1, scale = 1 / 7 onto a preloaded out (every forward step: the fwd_mean map)
    tokens = torch.tensor([[1, 2], [3, 4]], dtype=torch.int32).cuda()
    pre = torch.rand(2, 2, L, L, generator=torch.Generator().manual_seed(9))
    out = word_maps(capi, acc_d, res, L, tokens, 0, 0b11111, out=pre.cuda(), accumulate=1, scale=1.0 / 7.0)
    for img in range(2):
        for j in range(2):
            want = pre[img, j].double() + float(np.float32(1.0 / 7.0)) * ref(img, int(tokens[img, j]), sel=0)
            torch.testing.assert_close(out[img, j].double(), want, rtol=1e-4, atol=1e-5)
    # a token outside the 77-word context poisons its own plane and nothing else
    tokens = torch.tensor([[1, -1, 5], [77, 2, 3]], dtype=torch.int32).cuda()
    out = word_maps(capi, acc_d, res, L, tokens, 1, 0b11111)
    for img in range(2):
        for j in range(3):
            tok = int(tokens[img, j])
            if tok < 0 or tok >= 77:
                assert torch.isnan(out[img, j]).all()
            else:
                torch.testing.assert_close(out[img, j].double(), ref(img, tok), rtol=1e-4, atol=1e-5)


def test_word_maps_refusals(capi):
    acc, acc_d = map_store(6)
    tokens = torch.tensor([[1]], dtype=torch.int32).cuda()
    out = torch.zeros(24 * 24, device="cuda")
    lib = capi.load()
    args = lambda row_sel, lm, n_img=1: (capi.ptr(acc_d), 5, N_CAP, HEADS, 6, 24, n_img, capi.ptr(tokens), 1, STEPS, row_sel, lm, capi.ptr(out), 0, 1.0, capi.stream_ptr())
    assert lib.etainv_op_word_maps_ex(*args(0, 0b100000)) != 0 and b"no layer" in lib.etainv_last_error()      # a mask that selects no stored layer
    assert lib.etainv_op_word_maps_ex(*args(2, 0b11111)) != 0 and b"row_sel" in lib.etainv_last_error()
    assert lib.etainv_op_word_maps_ex(*args(0, 0b11111, n_img=N_CAP + 1)) != 0


BLEND_THRES = 0.3


def blend_inputs(res, L, seed):
    """LocalBlend inputs: image 0 has no blend words (alpha rows all zero), image 1 blends token 3 of the source and 4 of the target prompt"""
    acc, acc_d = map_store(res)
    x = torch.randn(4, 4, L, L, generator=torch.Generator().manual_seed(seed))
    alpha = torch.zeros(2, 2, 77)
    alpha[1, 0, 3] = alpha[1, 1, 4] = 1
    return acc, acc_d, x, alpha


def blend_ratios(acc, img, alpha, res):
    """pooled / max of LocalBlend.mask (oracle/ptp.py) in float64 at the store's resolution: what the threshold compares"""
    maps = torch.cat([acc[l, img].double().reshape(2, HEADS, 1, res, res, 77) for l in range(5)], dim=1)
    m = (maps * alpha[img].double().reshape(2, 1, 1, 1, 1, 77)).sum(-1).mean(1)
    m = F.max_pool2d(m, (3, 3), (1, 1), padding=(1, 1))
    return m / m.max(2, keepdim=True)[0].max(3, keepdim=True)[0]


@pytest.mark.parametrize("res,L", [(6, 24), (24, 96)])
def test_local_blend_sizes_untouched_image_and_mask(capi, res, L, monkeypatch):
    from oracle import ptp as optp
    lib = capi.load()
    acc, acc_d, x, alpha = blend_inputs(res, L, seed=21)
    # the threshold is a comparison: the reference decides every pixel with a margin (STORE_SEED was chosen on the CPU so that this holds)
    ratio = blend_ratios(acc, 1, alpha, res)
    assert float((ratio - float(np.float32(BLEND_THRES))).abs().min()) > 1e-4
    ad = alpha.cuda()
    xd = x.clone().cuda()
    capi.check(lib.etainv_op_local_blend(capi.ptr(acc_d), 5, N_CAP, HEADS, res, L, capi.ptr(xd), 2, capi.ptr(ad), BLEND_THRES, capi.stream_ptr()))
    torch.cuda.synchronize()
    got = xd.cpu()
    # image 0: no blend words -> both of its rows come back bit-identical, while image 1 is blended in the same launch
    assert torch.equal(bits(got[0]), bits(x[0])) and torch.equal(bits(got[2]), bits(x[2]))
    lb = optp.LocalBlend(alpha[1].numpy(), 10, res=res, th=BLEND_THRES)
    lb.counter = 100
    lay = [acc[l, 1].double().reshape(2 * HEADS, res * res, 77) for l in range(5)]
    store = {"down_cross": [None, None, lay[0], lay[1]], "up_cross": lay[2:]}
    pair = torch.stack([x[1], x[3]]).double()
    ref = lb(pair, store)
    assert torch.equal(bits(got[1]), bits(x[1])), "the source row is never written"
    torch.testing.assert_close(got[3].double(), ref[1], rtol=1e-6, atol=1e-6)
    on = lb.mask(pair, store)[1, 0]                                   # [L][L] bool: source mask | target mask
    assert 0 < int(on.sum()) < L * L
    off = ~on
    assert torch.equal(bits(got[3][:, off]), bits(x[1][:, off])), "target pixels outside the mask are the source row's, bit for bit"
    # the split partial sums (default) and the single loop (ETAINV_BLEND_NOSPLIT=1) give the same bits
    x2 = x.clone().cuda()
    monkeypatch.setenv("ETAINV_BLEND_NOSPLIT", "1")
    capi.check(lib.etainv_op_local_blend(capi.ptr(acc_d), 5, N_CAP, HEADS, res, L, capi.ptr(x2), 2, capi.ptr(ad), BLEND_THRES, capi.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(bits(x2), bits(xd))


# ----------------------------------------------------------------------------------------- edge kernels of the UNet
HALF_ULP = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def time_embedding(capi, t, dim, dtype):
    rows = len(t)
    t_host = (C.c_int64 * rows)(*[int(v) for v in t])
    out = guarded_flat(rows * dim, dtype, dim)
    capi.check(capi.load().etainv_op_time_embedding(t_host, rows, dim, capi.ptr(out), capi.dtype_code(dtype), capi.stream_ptr()))
    assert_guard(out, rows * dim)
    return out[:rows * dim].view(rows, dim)


def time_embedding_ref(t, dim):
    """diffusers get_timestep_embedding(flip_sin_to_cos=True, downscale_freq_shift=0) in float64: [cos | sin] of t * exp(-ln 10000 * k / half)"""
    half = dim // 2
    arg = torch.tensor(t, dtype=torch.float64)[:, None] * torch.exp(-np.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)[None]
    return torch.cat([torch.cos(arg), torch.sin(arg)], dim=1)


T_130 = ([999, 1, 3, 5, 7] + list(range(0, 1000, 8)))[::-1]      # 130 distinct timesteps, 0 and 999 among them


@pytest.mark.parametrize("dtype", DTYPES3)
@pytest.mark.parametrize("t", [[0] * 5, [1] * 5, [500] * 5, [981] * 5, [999] * 5, T_130],
                         ids=["t0", "t1", "t500", "t981", "t999", "rows130"])
def test_time_embedding(capi, dtype, t):
    """uniform rows (one scalar in the kernel arguments) and 130 distinct timesteps (chunks of 64 rows at row0 = 0, 64, 128, the last one ragged).
    Bound: the fp32 argument t * freq carries at most about 4
    roundings of 2^-24 relative on |a| <= 999, and d cos / da <= 1: atol = 999 * 4 * 2^-24 = 2.4e-4, plus half an ulp of the output type (|value| <= 1)."""
    dim = 320
    if len(t) == 130:
        assert len(set(t)) == 130 and max(t) == 999 and min(t) == 0
    out = time_embedding(capi, t, dim, dtype)
    err = (out.cpu().double() - time_embedding_ref(t, dim)).abs()
    bound = 999 * 4 * 2.0 ** -24 + HALF_ULP[dtype]
    print(f"time embedding {dtype} rows={len(t)} t0={t[0]}: max |err| {float(err.max()):.3e} (bound {bound:.3e})")
    assert float(err.max()) <= bound


@pytest.mark.parametrize("dtype", DTYPES3)
@pytest.mark.parametrize("inplace", [False, True])
def test_silu(capi, dtype, inplace):
    n = 3 * 1280 + 5
    x = urand(n, seed=1, lo=-12.0, hi=12.0, dtype=dtype)
    ref = x.cpu().double() * torch.sigmoid(x.cpu().double())
    buf = guarded_flat(n, dtype, 256)
    if inplace:
        buf[:n] = x
    capi.check(capi.load().etainv_op_silu(capi.ptr(buf) if inplace else capi.ptr(x), capi.ptr(buf), n, capi.dtype_code(dtype), capi.stream_ptr()))
    assert_guard(buf, n)
    close64(buf[:n], ref, ULP[dtype])


def cast_source(n, dtype):
    """values over the whole range of the types: ties, sub-normals of fp16, overflow to inf, signed zeros"""
    v = torch.randn(n, generator=torch.Generator().manual_seed(3)) * torch.logspace(-9, 5.5, n)
    v[:12] = torch.tensor([0.0, -0.0, 65504.0, 65520.0, 70000.0, -70000.0, 1e-8, 6e-8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -8, 3.0e38])
    return v.to(dtype).cuda()


@pytest.mark.parametrize("dst", DTYPES3)
@pytest.mark.parametrize("src", DTYPES3)
def test_cast(capi, src, dst):
    n = 4 * 256 + 37
    x = cast_source(n, src)
    out = guarded_flat(n, dst, 256)
    capi.check(capi.load().etainv_op_cast(capi.ptr(x), capi.dtype_code(src), capi.ptr(out), capi.dtype_code(dst), n, capi.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(out[n:], torch.full_like(out[n:], -777.0)), "the kernel wrote behind its output"
    assert torch.equal(bits(out[:n]), bits(x.cpu().to(dst)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("io", [torch.float32, torch.float16])
@pytest.mark.parametrize("L", [8, 12])
def test_im2col_in(capi, dtype, io, L):
    """the gather in front of conv_in's K = 64 GEMM: k = tap * 4 + ci, columns 36..63 zero, UNet row r reads latent r % n_lat (row 2 reads latent 0)"""
    n_lat, rows = 2, 3
    x = rnd(n_lat, 4, L, L, seed=1, dtype=io)
    out = guarded_flat(rows * L * L * 64, dtype, 64 * 8)
    capi.check(capi.load().etainv_op_im2col_in(capi.ptr(x), capi.dtype_code(io), n_lat, rows, L, capi.ptr(out), capi.dtype_code(dtype), capi.stream_ptr()))
    assert_guard(out, rows * L * L * 64)
    src = x.cpu().float()[[r % n_lat for r in range(rows)]]
    cols = F.unfold(src, 3, padding=1).view(rows, 4, 9, L * L).permute(0, 3, 2, 1).reshape(rows, L * L, 36)        # unfold's k = ci * 9 + tap -> tap * 4 + ci
    want = torch.cat([cols, torch.zeros(rows, L * L, 28)], dim=2).to(dtype)
    got = out[:rows * L * L * 64].view(rows, L * L, 64)
    assert torch.equal(bits(got), bits(want))
    assert int(bits(got[..., 36:]).abs().max()) == 0


def pack(capi, src, rows, cols, mode, taps, dtype, scale=1.0, colscale=None, n_dst=None):
    n_dst = n_dst or rows * cols
    dst = guarded_flat(n_dst, dtype, 256)
    capi.check(capi.load().etainv_op_pack_weight(capi.ptr(src), capi.ptr(dst), rows, cols, mode, taps, scale, capi.ptr(colscale), capi.dtype_code(dtype),
                                                 capi.stream_ptr()))
    assert_guard(dst, n_dst)
    return dst[:n_dst].cpu()


@pytest.mark.parametrize("dtype", DTYPES3)
def test_pack_weight(capi, dtype):
    """an fp32 destination is the permuted source bit for bit; a 16-bit one is ((src * scale) * colscale).to(dtype), the product formed in that order in fp32"""
    scaled = lambda w, scale, cs=None: ((w.cpu() * scale) * cs.cpu()[None] if cs is not None else w.cpu() * scale).to(dtype)
    # mode 0: [130][70]
    w = rnd(130, 70, seed=1)
    cs = 1.0 + 0.3 * rnd(70, seed=2)
    assert torch.equal(bits(pack(capi, w, 130, 70, 0, 1, dtype).view(130, 70)), bits(scaled(w, 1.0)))
    assert torch.equal(bits(pack(capi, w, 130, 70, 0, 1, dtype, 0.37, cs).view(130, 70)), bits(scaled(w, 0.37, cs)))
    assert torch.equal(bits(pack(capi, w, 130, 70, 0, 1, dtype, 0.37).view(130, 70)), bits(scaled(w, 0.37)))
    # mode 1: conv OIHW [O = 5][I = 12][3][3] -> [O][tap][I]
    w = rnd(5, 12, 3, 3, seed=3)
    assert torch.equal(bits(pack(capi, w, 5, 12 * 9, 1, 9, dtype).view(5, 9, 12)), bits(scaled(w.view(5, 12, 9).permute(0, 2, 1).contiguous(), 1.0)))
    # mode 2: GEGLU row interleave of [256][40]
    w = rnd(256, 40, seed=4)
    cs = 1.0 + 0.3 * rnd(40, seed=5)
    assert torch.equal(bits(pack(capi, w, 256, 40, 2, 1, dtype).view(256, 40)), bits(pack_geglu(scaled(w, 1.0))))
    assert torch.equal(bits(pack(capi, w, 256, 40, 2, 1, dtype, 0.37, cs).view(256, 40)), bits(pack_geglu(scaled(w, 0.37, cs))))
    # mode 5: conv_in [O = 24][4][3][3] -> [O][64], k = tap * 4 + ci, zero from 36 on
    w = rnd(24, 4, 3, 3, seed=6)
    want = torch.cat([w.cpu().view(24, 4, 9).permute(0, 2, 1).reshape(24, 36), torch.zeros(24, 28)], dim=1).to(dtype)
    assert torch.equal(bits(pack(capi, w, 24, 36, 5, 9, dtype, n_dst=24 * 64).view(24, 64)), bits(want))


def test_pack_weight_refusals(capi):
    lib = capi.load()
    w, cs = rnd(5, 12 * 9, seed=1), rnd(12 * 9, seed=2)
    dst = torch.zeros(5 * 12 * 9, device="cuda")
    call = lambda mode, colscale, rows=5, cols=12 * 9, taps=9: lib.etainv_op_pack_weight(capi.ptr(w), capi.ptr(dst), rows, cols, mode, taps, 1.0, capi.ptr(colscale),
                                                                                         capi.F32, capi.stream_ptr())
    assert call(1, cs) != 0 and b"column scale" in lib.etainv_last_error()        # a per-column factor of a permuted conv weight is not defined
    for retired in (3, 4):                                                      # the layouts of the retired direct conv_in / conv_out kernels
        assert call(retired, None) != 0 and b"pack mode" in lib.etainv_last_error()
    assert call(2, None) != 0                                                   # GEGLU interleave of 5 rows
    assert call(1, None, taps=7) != 0
    assert call(5, None, cols=40) != 0 and b"conv_in packing" in lib.etainv_last_error()      # mode 5 reads 36 values per row whatever cols says
    torch.cuda.synchronize()
    assert float(dst.abs().max()) == 0.0


_TPROJ = {}


def tproj_operands(dtype):
    """the UNet's time projections as one GEMM: N = 20160 = the sum of the 22 ResnetBlock2D.time_emb_proj widths, K = 1280 (the largest tensor of this file)"""
    if dtype not in _TPROJ:
        n, k = 20160, 1280
        _TPROJ[dtype] = (rnd(n, k, seed=2, scale=k ** -0.5, dtype=dtype), rnd(n, seed=3))
    return _TPROJ[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1, 3, 16, 128])
def test_gemm_f32out_time_projections(capi, dtype, m):
    n, k = 20160, 1280
    w, bias = tproj_operands(dtype)
    a = rnd(m, k, seed=1, dtype=dtype)
    out = torch.full((m + 1, n), NAN, device="cuda")
    capi.check(capi.load().etainv_op_gemm_f32out(capi.ptr(a), capi.ptr(w), capi.ptr(bias), capi.ptr(out), m, n, k, capi.dtype_code(dtype), capi.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.isnan(out[m]).all(), "the guard row behind M was written"
    ref = a.float() @ w.float().t() + bias
    assert relerr(out[:m], ref) < TOL[dtype]
    d, r = (out[:m] - ref).reshape(m, n // 160, 160), ref.reshape(m, n // 160, 160)
    blk = d.norm(dim=(0, 2)) / r.norm(dim=(0, 2))
    assert float(blk.max()) < 2 * TOL[dtype], f"worst 160-column block: {int(blk.argmax())}"


TPROJ_N, TPROJ_COL = 20160, 5440


def conv_rv(capi, x_nhwc, wk, bias, rowvec, res, b, h, wd, cin, cout, stride, ups, dtype, strided):
    """etainv_op_conv3x3_rv with the time row either as its own [b][cout] matrix or as columns 5440.. of a NaN-filled [b][20160] matrix (the UNet's form)"""
    ho, wo = (h * 2, wd * 2) if ups else ((h // 2, wd // 2) if stride == 2 else (h, wd))
    out = torch.full((b, ho, wo, cout), NAN, dtype=dtype, device="cuda")
    if strided:
        big = torch.full((b, TPROJ_N), NAN, device="cuda")
        big[:, TPROJ_COL:TPROJ_COL + cout] = rowvec
        rv, rvs = big.data_ptr() + 4 * TPROJ_COL, TPROJ_N
    else:
        big, rv, rvs = None, capi.ptr(rowvec), cout
    capi.check(capi.load().etainv_op_conv3x3_rv(capi.ptr(x_nhwc), None, cin, 0, capi.ptr(wk), capi.ptr(bias), rv, rvs, capi.ptr(res), capi.ptr(out), b, h, wd, cout,
                                                stride, ups, 9, capi.dtype_code(dtype), capi.stream_ptr()))
    torch.cuda.synchronize()
    return out


def conv_rv_inputs(dtype, b, h, wd, cin, cout, stride=1, ups=0, res=False):
    x = rnd(b, cin, h, wd, seed=1, dtype=dtype)
    w = rnd(cout, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5, dtype=dtype)
    bias, rowvec = rnd(cout, seed=3), rnd(b, cout, seed=5)
    xin = F.interpolate(x.float(), scale_factor=2.0, mode="nearest") if ups else x.float()
    ref = F.conv2d(xin, w.float(), bias, stride=stride, padding=1) + rowvec[:, :, None, None]
    r = rnd(b, ref.shape[2], ref.shape[3], cout, seed=6, dtype=dtype) if res else None
    if res:
        ref = ref + r.float().permute(0, 3, 1, 2)
    return dict(x_nhwc=x.permute(0, 2, 3, 1).contiguous(), wk=w.permute(0, 2, 3, 1).contiguous(), bias=bias, rowvec=rowvec, r=r, ref=ref,
                shape=(b, h, wd, cin, cout, stride, ups), dtype=dtype)


def conv_rv_check(capi, inp):
    """against F.conv2d + the row, in the strided form; and that form bit for bit against the dense one"""
    x_nhwc, wk, bias, rowvec, r, ref, dtype = (inp[k] for k in ("x_nhwc", "wk", "bias", "rowvec", "r", "ref", "dtype"))
    b, h, wd, cin, cout, stride, ups = inp["shape"]
    got = conv_rv(capi, x_nhwc, wk, bias, rowvec, r, b, h, wd, cin, cout, stride, ups, dtype, strided=True)
    assert relerr(got.permute(0, 3, 1, 2), ref) < TOL[dtype]           # (one NaN column read instead of the row's makes this NaN)
    per_image = (got.float().permute(0, 3, 1, 2) - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)
    assert float(per_image.max()) < 2 * TOL[dtype]                      # a row of another image hides in a global norm
    plain = conv_rv(capi, x_nhwc, wk, bias, rowvec, r, b, h, wd, cin, cout, stride, ups, dtype, strided=False)
    assert torch.equal(got, plain), "the same launch with a dense [b][cout] time row"
    return got


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv3x3_strided_time_row_patch_routes(capi, dtype, monkeypatch):
    """the stride-1 convs at (16, 64, 64, 320, 320) (tests/test_kernels_gpu.py test_conv3x3_ping_pong_patch) under the three settings of ETAINV_PPCONV /
    ETAINV_PPCONV2: ppconv.hip's dual-M form, its 256-pixel form and igemm.hip's PATCH ring.  As in that test: the 256-pixel form and the ring agree bit
    for bit, the dual-M form within one ulp of the stored type."""
    inp = conv_rv_inputs(dtype, 16, 64, 64, 320, 320, res=True)
    outs = []
    for pp, pp2 in (("1", "1"), ("1", "0"), ("0", "0")):
        monkeypatch.setenv("ETAINV_PPCONV", pp)
        monkeypatch.setenv("ETAINV_PPCONV2", pp2)
        outs.append(conv_rv_check(capi, inp))
    assert torch.equal(outs[1], outs[2])
    one_ulp = 2.0 ** (-7 if dtype == torch.bfloat16 else -10)
    assert float(((outs[0].float() - outs[2].float()).abs() / outs[2].float().abs().clamp_min(0.25)).max()) <= 1.01 * one_ulp


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", [dict(b=4, h=32, wd=32, cin=320, cout=320, res=True),              # 32 output tiles, below the 192 from which a conv goes to
                                                                                                   # ppconv.hip: igemm.hip's kernel, the UNet's route at batch 1
                                 dict(b=1, h=8, wd=8, cin=1280, cout=1280, res=True),              # split-K: the reduction kernel adds the row
                                 dict(b=2, h=16, wd=16, cin=640, cout=640, stride=2, res=True),    # stride 2
                                 dict(b=1, h=16, wd=16, cin=640, cout=640, ups=1, res=True),       # nine taps behind the fused upsample
                                 dict(b=3, h=12, wd=12, cin=320, cout=64, res=True),               # ragged tiles
                                 dict(b=2, h=8, wd=8, cin=1280, cout=1280, res=True),              # (with one image the stride is never multiplied:
                                 dict(b=2, h=16, wd=16, cin=640, cout=640, ups=1, res=True)],      #  the two single-image routes again with two)
                         ids=["small_m", "split_k", "stride2", "upsample9", "ragged", "split_k_b2", "upsample9_b2"])
def test_conv3x3_strided_time_row_other_routes(capi, dtype, cfg):
    conv_rv_check(capi, conv_rv_inputs(dtype, **cfg))


def test_conv3x3_rv_refusal(capi):
    x, w, bias, rowvec = rnd(1, 8, 8, 64, seed=1, dtype=torch.float16), rnd(64, 3, 3, 64, seed=2, dtype=torch.float16), rnd(64, seed=3), rnd(1, 64, seed=4)
    out = torch.zeros(1, 8, 8, 64, dtype=torch.float16, device="cuda")
    lib = capi.load()
    assert lib.etainv_op_conv3x3_rv(capi.ptr(x), None, 64, 0, capi.ptr(w), capi.ptr(bias), capi.ptr(rowvec), 63, None, capi.ptr(out), 1, 8, 8, 64, 1, 0, 9, capi.F16,
                                    capi.stream_ptr()) != 0
    assert b"rowvec_stride" in lib.etainv_last_error()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b,hw,c", [(3, 256, 320), (2, 1024, 640)])
def test_groupnorm_fold_and_per_image_gemm(capi, dtype, b, hw, c):
    """Transformer2DModel.norm folded into proj_in: etainv_op_gn_fold makes one weight matrix and one bias per image, etainv_op_gemm_per_image applies them to
    the RAW rows.  Against GroupNorm(32, eps 1e-6)(x) W^T + bias in fp32.  The images have distinct statistics with means well away from zero: the weight
    matrix of another image then shows in that image's error (it is invisible in a global norm when the statistics agree)."""
    lib, dt, groups, eps = capi.load(), capi.dtype_code(dtype), 32, 1e-6
    mu, sigma = [1.5, -2.0, 1.2][:b], [1.0, 0.6, 1.7][:b]
    x = torch.stack([rnd(hw, c, seed=10 + i, scale=sigma[i]).float() + mu[i] + 0.5 * rnd(c, seed=20 + i)[None] for i in range(b)]).to(dtype).contiguous()
    w = rnd(c, c, seed=1, scale=c ** -0.5)
    gamma, beta, bias = 1.0 + 0.3 * rnd(c, seed=2), 0.2 * rnd(c, seed=3), rnd(c, seed=4)
    xg = x.double().view(b, hw, groups, c // groups)
    mean, var = xg.mean(dim=(1, 3)), xg.var(dim=(1, 3), unbiased=False)
    stats = torch.stack([mean, (var + eps).rsqrt()], dim=-1).float().contiguous()            # [b][groups] (mean, rstd), as launch_gn_finalize leaves them
    assert float((mean.abs().min(dim=1).values).min()) > 0.3 and float((stats[:, :, 1].mean(1)[0] / stats[:, :, 1].mean(1)[1] - 1).abs()) > 0.2
    wb = guarded_flat(b * c * c, dtype, 1024)
    cb = guarded_flat(b * c, torch.float32, 64)
    capi.check(lib.etainv_op_gn_fold(capi.ptr(w), capi.ptr(gamma), capi.ptr(beta), capi.ptr(bias), capi.ptr(stats), groups, b, c, c, capi.ptr(wb), capi.ptr(cb), dt,
                                     capi.stream_ptr()))
    assert_guard(wb, b * c * c)
    assert_guard(cb, b * c)
    cpg = c // groups
    a = stats[:, :, 1].repeat_interleave(cpg, dim=1) * gamma[None]                            # [b][k] fp32: rstd * gamma
    # wb = W * a rounded to the compute dtype, bit for bit.  The product of two fp32 numbers is exact in float64; (W * a).to(dtype) rounds it to fp32 and
    # then to dtype.  The bf16 kernel does exactly that.  The fp16 kernel's multiply and conversion are one instruction on gfx950 (v_fma_mixlo_f16), which
    # rounds the exact product ONCE: 17 of the 307200 elements at (3, 256, 320) and 47 of 819200 at (2, 1024, 640) sit at a double-rounding tie and
    # differ from the twice-rounded value.  Each type is pinned to its rounding, so a change of either shows.
    wb_ref = round_once(w.double()[None] * a.double()[:, None, :], dtype) if dtype == torch.float16 else (w[None] * a[:, None, :]).to(dtype).cpu()
    assert torch.equal(bits(wb[:b * c * c].view(b, c, c)), bits(wb_ref))
    # cb[b][n] = sum_k (beta[k] W[n][k] - mean[b][g(k)] * the ROUNDED weight wb_ref[b][n][k]) + bias[n] in float64 (wb_ref is the reference just checked
    # bit for bit, not the kernel's output): rtol 1e-4.  The sum cancels (|cb| from 4e-5 to 9 over these cases), so rtol alone cannot hold: the same
    # expression summed in fp32 torch is off float64 by at most 1.7e-6 over the four cases of this test (measured on the CPU); atol is twice that, 3.4e-6.
    mean_k = stats[:, :, 0].double().repeat_interleave(cpg, dim=1).cpu()
    cb_ref = (beta.double().cpu()[None, None] * w.double().cpu()[None] - mean_k[:, None, :] * wb_ref.double()).sum(-1) + bias.double().cpu()[None]
    cb_err = (cb[:b * c].view(b, c).cpu().double() - cb_ref).abs()
    print(f"gn_fold {dtype} ({b}, {hw}, {c}): cb off by at most {float(cb_err.max()):.3e}")
    assert bool((cb_err <= 1e-4 * cb_ref.abs() + 2 * 1.7e-6).all())
    out = torch.full((b * hw + 64, c), NAN, dtype=dtype, device="cuda")
    capi.check(lib.etainv_op_gemm_per_image(capi.ptr(x), capi.ptr(wb), capi.ptr(cb), None, capi.ptr(out), b, hw, c, c, dt, capi.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.isnan(out[b * hw:]).all()
    xn = F.group_norm(x.float().permute(0, 2, 1), groups, gamma, beta, eps).permute(0, 2, 1)
    ref = xn @ w.t() + bias
    got = out[:b * hw].view(b, hw, c)
    assert relerr(got, ref) < TOL[dtype]
    per_image = (got.float() - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)
    assert float(per_image.max()) < 2 * TOL[dtype], per_image
    # a tile that would span two images is refused, not computed with one image's weights
    bad = torch.zeros(2 * 100, c, dtype=dtype, device="cuda")
    assert lib.etainv_op_gemm_per_image(capi.ptr(x), capi.ptr(wb), capi.ptr(cb), None, capi.ptr(bad), 2, 100, c, c, dt, capi.stream_ptr()) != 0
    assert b"per-image weights" in lib.etainv_last_error()
