"""etainv_prox_guidance (csrc/proximal.hip): the two selected order statistics bit for bit against torch.sort, the threshold against their
float64 interpolation, the l0 result per element against float64 on the kernel's own threshold, the l1 result bit for bit against the fp32
restatement of the reference's three lines, over sizes on every code path (registers with 4 and 32 values per thread, values in eps_out) and
input regimes built around ties.

Bounds.  v_k, v_k+1: equality (|eps_c - eps_u| is one exact IEEE subtraction and a sign flip on both sides; selection rounds nothing).
thr: 2 ulp(v_k+1) -- three roundings (difference, product, sum) of at most half an ulp of magnitudes up to v_k+1.
l0, per element: g ulp(D) + ulp(g D) / 2 + ulp(O) / 2, D the group's largest |d|, O its largest |out|: the subtraction and the shrink round
once each (half an ulp of D, times g), the product and the sum once each.
l1 with eps_u = 0, g = 1: equality -- d = eps_c, the product and the sum are exact, the three lines round where torch's fp32 lines round.

Measured on MI355X (this file's own printouts): see DESIGN.md, "Proximal guidance"."""
import numpy as np
import pytest
import torch

from tests import regdiff_ref as rr

pytestmark = pytest.mark.gpu
G = 7.5
SIZES = [(8, 1), (8, 2), (20, 2), (44, 3), (64, 2), (96, 2), (96, 4)]            # (l, rows per group)
REGIMES = ["white", "zero_row", "eighths", "equal", "low8", "exponent", "denormal"]
RANKS = ["q0.7", "k0", "q1", "straddle", "inside_run"]


def rank_split(n, q):
    from etainv.pipeline import ProximalGuidance
    return ProximalGuidance.rank_split(n, q)


def run(u, c, g, mode, n_groups, k=None, w=0.0, thr=0.0, x=None, a_from=1.0, a_to=1.0, out=None, want_thr=True):
    """one call of the entry point; u, c (rows_per_group * n_groups, 4, l, l) device tensors, tensor row r * n_groups + j = row r of group j.
    k None: the fixed threshold `thr`.  Returns (eps_out, thr_out (n_groups, 3) or None, x_out)"""
    from etainv import _capi
    rows, _, l, _ = u.shape
    out = torch.empty_like(c) if out is None else out
    x_out = torch.empty_like(x) if x is not None else None
    thr_out = torch.full((n_groups, 3), -1.0, device="cuda") if want_thr else None
    _capi.check(_capi.load().etainv_prox_guidance(_capi.ptr(u), _capi.ptr(c), float(g), mode, int(k is not None), int(k or 0), float(w), float(thr),
                                                  _capi.ptr(out), _capi.ptr(x), float(a_from), float(a_to), _capi.ptr(x_out), _capi.ptr(thr_out),
                                                  n_groups, rows // n_groups, l, _capi.stream_ptr()))
    torch.cuda.synchronize()
    return out, thr_out, x_out


def inputs(kind, l, rows, n_groups, seed):
    """(eps_u, eps_c) fp32 CPU tensors (rows * n_groups, 4, l, l); every group gets its own draws"""
    gen = torch.Generator().manual_seed(seed)
    shape = (rows * n_groups, 4, l, l)
    n = int(np.prod(shape))
    u, c = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    bits = lambda b: torch.from_numpy(b.astype(np.uint32).view(np.float32).reshape(shape).copy())
    rnd = lambda hi: torch.randint(0, hi, (n,), generator=gen).numpy()
    if kind == "zero_row":                                       # the first row of every group: d exactly zero
        c[:n_groups] = u[:n_groups]
    elif kind == "eighths":
        u, c = torch.round(u * 8) / 8, torch.round(c * 8) / 8
    elif kind == "equal":                                        # every d the same value (u, u + 0.5 exact in eighths)
        u = torch.round(u * 8) / 8
        c = u + 0.5
    elif kind == "low8":                                         # |d| patterns differ in their lowest 8 bits only; both signs
        u, c = torch.zeros(shape), bits(0x3f9a2b00 | rnd(256) | (rnd(2).astype(np.uint32) << 31))
    elif kind == "exponent":                                     # |d| = 2^e: the patterns differ in the exponent only
        u, c = torch.zeros(shape), bits(((87 + rnd(80)).astype(np.uint32) << 23) | (rnd(2).astype(np.uint32) << 31))
    elif kind == "denormal":                                     # denormals of both signs, a third of the values +0.0 or -0.0
        m = rnd(1 << 23) * (rnd(3) > 0)
        u, c = torch.zeros(shape), bits(m.astype(np.uint32) | (rnd(2).astype(np.uint32) << 31))
    elif kind != "white":
        raise ValueError(kind)
    return u.contiguous(), c.contiguous()


def group_rows(t, j, n_groups):
    return t[j::n_groups]


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def shrink32(d, thr, l1):
    """the reference's lines in fp32 torch on the CPU"""
    t = torch.tensor(float(thr), dtype=torch.float32)
    s = d - d.clamp(-t, t)
    if l1:
        s = torch.where(s > 0, s - t, s)
        s = torch.where(s < 0, s + t, s)
    return s


def check_case(u, c, n_groups, k, w, what):
    """everything the module docstring lists, for one input and one rank"""
    rows = u.shape[0] // n_groups
    out, thr_out, _ = run(u.cuda(), c.cuda(), G, 1, n_groups, k, w)
    d32 = c - u                                                  # fp32 on the CPU: the same exact IEEE subtraction
    out1, thr1, _ = run(torch.zeros_like(d32).cuda(), d32.cuda(), 1.0, 2, n_groups, k, w)
    out, thr_out, out1, thr1 = out.cpu(), thr_out.cpu(), out1.cpu(), thr1.cpu()
    assert torch.equal(thr_out.view(torch.int32), thr1.view(torch.int32))          # same d, same rank: the same selection in both launches
    worst = 0.0
    for j in range(n_groups):
        dj, uj = group_rows(d32, j, n_groups), group_rows(u, j, n_groups)
        s = torch.sort(dj.abs().flatten()).values
        n = s.numel()
        assert n == rows * 4 * u.shape[2] ** 2
        thr, vk, vk1 = thr_out[j]
        want_k, want_k1 = s[k], s[min(k + 1, n - 1)]
        assert vk.view(torch.int32) == want_k.view(torch.int32) and vk1.view(torch.int32) == want_k1.view(torch.int32), (what, j, vk, want_k, vk1, want_k1)
        thr64 = float(want_k) + float(w) * (float(want_k1) - float(want_k))
        assert abs(float(thr) - thr64) <= 2 * ulp32(float(want_k1)), (what, j, float(thr), thr64)
        # l0 against float64 on the kernel's own threshold
        u64, t64 = uj.double().numpy(), float(thr)
        d64 = group_rows(c, j, n_groups).double().numpy() - u64
        want = u64 + G * (d64 - np.clip(d64, -t64, t64))
        D, O = np.abs(d64).max(), np.abs(want).max()
        bound = G * ulp32(D) + ulp32(G * D) / 2 + ulp32(O) / 2
        err = np.abs(group_rows(out, j, n_groups).double().numpy() - want).max()
        worst = max(worst, err / bound)
        assert err <= bound, (what, j, err, bound)
        # l1, eps_u = 0, g = 1: bit for bit
        want1 = shrink32(dj, thr, True)
        got1 = group_rows(out1, j, n_groups)
        assert np.array_equal(got1.numpy(), want1.numpy()), (what, j, np.abs(got1 - want1).max())
    print(f"{what}: l0 max error at {worst:.2f} of its bound")


@pytest.mark.parametrize("n_groups", [1, 3])
@pytest.mark.parametrize("l,rows", SIZES)
def test_sizes(l, rows, n_groups):
    u, c = inputs("white", l, rows, n_groups, seed=1000 + 10 * l + rows)
    k, w = rank_split(rows * 4 * l * l, 0.7)
    check_case(u, c, n_groups, k, w, f"l = {l} rows = {rows} n_groups = {n_groups} white q = 0.7 (k = {k}, w = {w:.4f})")


@pytest.mark.parametrize("regime", REGIMES[1:])
@pytest.mark.parametrize("l,rows", [(20, 2), (64, 2)])
def test_input_regimes(l, rows, regime):
    n_groups, n = 3, rows * 4 * l * l
    u, c = inputs(regime, l, rows, n_groups, seed=2000 + 10 * l + REGIMES.index(regime))
    for q in (0.7, 0.3):
        k, w = rank_split(n, q)
        check_case(u, c, n_groups, k, w, f"l = {l} {regime} q = {q}")


@pytest.mark.parametrize("rank", RANKS[1:])
@pytest.mark.parametrize("l,rows", [(20, 2), (64, 2), (96, 4)])
def test_ranks(l, rows, rank):
    """k = 0; q = 1 (k = n - 1 = k + 1's clamp); k and k + 1 on two distinct values; both inside a run of equal values -- on d in eighths (runs of
    hundreds of equal values) and, for the first two, on white noise as well"""
    n_groups, n = 1, rows * 4 * l * l
    u, c = inputs("eighths", l, rows, n_groups, seed=3000 + l)
    s = torch.sort((c - u).abs().flatten()).values
    if rank == "k0":
        cases = [(0, 0.5), (0, 0.0)]
    elif rank == "q1":
        cases = [rank_split(n, 1.0)]
        assert cases[0] == (n - 1, 0.0)
    else:
        steps = torch.nonzero(s[1:] > s[:-1]).flatten()          # k with s[k] < s[k + 1]
        assert len(steps) >= 3
        if rank == "straddle":
            cases = [(int(steps[len(steps) // 2]), 0.25), (int(steps[0]), 0.75), (int(steps[-1]), 0.5)]
            assert all(s[k] < s[k + 1] for k, _ in cases)
        else:
            mid = int(steps[len(steps) // 2])
            cases = [(mid + 1, 0.5), (mid - 1, 0.25), (int(steps[0]) // 2, 0.75)]      # first of a run, last but one of a run, inside the first run
            assert all(s[k] == s[k + 1] for k, _ in cases)
    for k, w in cases:
        check_case(u, c, n_groups, k, w, f"l = {l} eighths {rank} (k = {k}, w = {w})")
        if rank in ("k0", "q1"):
            uw, cw = inputs("white", l, rows, n_groups, seed=3100 + l)
            check_case(uw, cw, n_groups, k, w, f"l = {l} white {rank} (k = {k}, w = {w})")


@pytest.mark.parametrize("l,rows", [(20, 2), (64, 2), (96, 2)])
def test_fixed_threshold_and_pass_through(l, rows):
    n_groups = 2
    u, c = inputs("white", l, rows, n_groups, seed=4000 + l)
    ud, cd = u.cuda(), c.cuda()
    cfg = u + G * (c - u)                                        # fp32 torch on the CPU: one rounding per operation, no contraction
    out0, thr0, _ = run(ud, cd, G, 1, n_groups, thr=0.0)         # quantile 0: the fixed threshold 0 -- plain CFG
    assert np.array_equal(out0.cpu().numpy(), cfg.numpy()) and not thr0.any()
    plain, thrp, _ = run(ud, cd, G, 0, n_groups, k=5, w=0.5, thr=3.0)                  # mode 0 ignores rank and threshold
    assert torch.equal(plain.view(torch.int32), out0.view(torch.int32)) and not thrp.any()
    for mode in (1, 2):
        out, thr_out, _ = run(ud, cd, G, mode, n_groups, thr=0.25)
        assert torch.equal(thr_out.cpu(), torch.full((n_groups, 3), 0.25))
        if mode == 1:                                            # l0 against float64, at the bound of the module docstring
            u64 = u.double().numpy()
            d64 = c.double().numpy() - u64
            want = u64 + G * (d64 - np.clip(d64, -0.25, 0.25))
            bound = G * ulp32(np.abs(d64).max()) + ulp32(G * np.abs(d64).max()) / 2 + ulp32(np.abs(want).max()) / 2
            assert np.abs(out.cpu().double().numpy() - want).max() <= bound
        want32 = u + G * shrink32(c - u, 0.25, mode == 2)        # and both bit for bit against the fp32 lines (nothing is contracted)
        assert np.array_equal(out.cpu().numpy(), want32.numpy()), mode
    no_thr, _, _ = run(ud, cd, G, 1, n_groups, thr=0.25, want_thr=False)               # thr_out may be NULL
    assert torch.equal(no_thr, run(ud, cd, G, 1, n_groups, thr=0.25)[0])


def test_nan_in_one_group_of_three():
    l, rows, n_groups = 20, 2, 3
    n = rows * 4 * l * l
    k, w = rank_split(n, 0.7)
    u, c = inputs("white", l, rows, n_groups, seed=5000)
    c[4, 2, 7, 3] = float("inf")                                 # group 1, its second row: +inf sorts last and poisons nothing at this rank
    clean, thr_clean, _ = run(u.cuda(), c.cuda(), G, 1, n_groups, k, w)
    assert torch.isfinite(thr_clean).all() and torch.isfinite(clean).sum() == clean.numel() - 1 and clean[4, 2, 7, 3] == float("inf")
    s = torch.sort((c - u)[1::n_groups].abs().flatten()).values
    assert s[-1] == float("inf") and torch.equal(thr_clean[1, 1:].cpu(), s[k:k + 2])
    c2 = c.clone()
    c2[1, 0, 0, 0] = float("nan")                                # group 1, its first row
    out, thr_out, _ = run(u.cuda(), c2.cuda(), G, 1, n_groups, k, w)
    assert torch.isnan(group_rows(out, 1, n_groups)).all() and torch.isnan(thr_out[1, 0])
    for j in (0, 2):
        assert torch.equal(group_rows(out, j, n_groups).view(torch.int32), group_rows(clean, j, n_groups).view(torch.int32))
        assert torch.equal(thr_out[j].view(torch.int32), thr_clean[j].view(torch.int32))


@pytest.mark.parametrize("l,rows", [(20, 2), (64, 2), (96, 4)])
def test_position_independence_repeatability_alias(l, rows):
    n_groups, n = 3, rows * 4 * l * l
    k, w = rank_split(n, 0.7)
    u, c = inputs("eighths" if l == 20 else "white", l, rows, n_groups, seed=6000 + l)
    ud, cd = u.cuda(), c.cuda()
    bits = lambda t: t.view(torch.int32)
    for mode in (1, 2):
        out, thr_out, _ = run(ud, cd, G, mode, n_groups, k, w)
        again, thr_again, _ = run(ud, cd, G, mode, n_groups, k, w)
        assert torch.equal(bits(out), bits(again)) and torch.equal(bits(thr_out), bits(thr_again))
        for j in range(n_groups):                                # a group of the three-group call == its single-group call
            one, thr_one, _ = run(group_rows(ud, j, n_groups).contiguous(), group_rows(cd, j, n_groups).contiguous(), G, mode, 1, k, w)
            assert torch.equal(bits(one), bits(group_rows(out, j, n_groups))) and torch.equal(bits(thr_one[0]), bits(thr_out[j]))
        flip = lambda t: t.reshape(rows, n_groups, *t.shape[1:]).flip(1).reshape(t.shape).contiguous()
        fl, thr_fl, _ = run(flip(ud), flip(cd), G, mode, n_groups, k, w)
        assert torch.equal(bits(flip(fl)), bits(out)) and torch.equal(bits(thr_fl.flip(0)), bits(thr_out))
        alias = cd.clone()                                       # eps_out may be eps_c
        res, thr_alias, _ = run(ud, alias, G, mode, n_groups, k, w, out=alias)
        assert res.data_ptr() == alias.data_ptr() and torch.equal(bits(alias), bits(out)) and torch.equal(bits(thr_alias), bits(thr_out))


@pytest.mark.parametrize("l,rows", [(20, 2), (64, 2), (96, 2)])
def test_fused_step(l, rows):
    """the DDIM step on the returned noise: against float64 on that noise, six roundings of half an ulp (4.8e-7) of values below 8
    (tests/test_regdiff_kernel_gpu.py::test_pass_through); the noise itself is bit-equal to the call without the step"""
    n_groups, n = 2, rows * 4 * l * l
    k, w = rank_split(n, 0.7)
    u, c = inputs("white", l, rows, n_groups, seed=7000 + l)
    lat = (0.5 * torch.randn(u.shape, generator=torch.Generator().manual_seed(7100 + l)) + 0.1).contiguous()
    for mode in (0, 1, 2):
        g = 1.625
        out, thr_out, stepped = run(u.cuda(), c.cuda(), g, mode, n_groups, k, w, x=lat.cuda(), a_from=0.8, a_to=0.9)
        alone, thr_alone, none = run(u.cuda(), c.cuda(), g, mode, n_groups, k, w)
        assert none is None and torch.equal(out.view(torch.int32), alone.view(torch.int32)) and torch.equal(thr_out, thr_alone)
        assert out.abs().max() < 8 and lat.abs().max() < 4
        want = rr.ddim_inverse_step(lat.double().numpy(), out.double().cpu().numpy(), 0.8, 0.9)
        assert np.abs(want).max() < 8
        err = np.abs(stepped.double().cpu().numpy() - want).max()
        print(f"l = {l} mode {mode}: fused step max-abs error {err:.3e} (bound 2e-6)")
        assert err <= 2e-6


def test_refusals_launch_nothing():
    """every refusal is an error code before anything is launched: the output keeps its fill"""
    from etainv import _capi
    u, c = (t.cuda() for t in inputs("white", 8, 1, 1, seed=8000))
    lib = _capi.load()
    out = torch.full_like(c, 123.0)
    thr_out = torch.full((1, 3), 123.0, device="cuda")

    def call(rows=1, l=8, k=10, w=0.5):
        return lib.etainv_prox_guidance(_capi.ptr(u), _capi.ptr(c), G, 1, 1, k, w, 0.0, _capi.ptr(out), None, 1.0, 1.0, None, _capi.ptr(thr_out), 1, rows, l,
                                        _capi.stream_ptr())
    for kw, fragment in ((dict(l=7), "[8, 96]"), (dict(l=97), "[8, 96]"), (dict(rows=5), "[1, 4]"), (dict(k=256), "[0, n - 1]"), (dict(k=-1), "[0, n - 1]")):
        assert call(**kw) != 0 and fragment in lib.etainv_last_error().decode(), kw
        torch.cuda.synchronize()
        assert (out == 123.0).all() and (thr_out == 123.0).all(), kw
    assert call(k=255, w=0.0) == 0                               # the last rank is a rank
    torch.cuda.synchronize()
    assert not (out == 123.0).any() and thr_out[0, 1] == (c - u).abs().max()
