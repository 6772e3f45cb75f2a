"""tests/proxnpi_ref.py (the restatement of negative-prompt inversion and proximal guidance that the GPU tests compare the engine with) against
fixtures recorded from the reference implementation's own classes (tests/golden/make_proxnpi_golden.py --reference), its rank split against
torch.quantile, the l1 rule's table, and the half-zero consequence.  CPU only."""
import numpy as np
import pytest
import torch

from tests import proxnpi_ref as pr
from tests.golden.make_proxnpi_golden import (E2E_L, E2E_S, GUIDANCE_CASES, GUIDANCE_G, GUIDANCE_SETTINGS, VARIANTS, guidance_keep,
                                              guidance_key)

# every n = rows * 4 * l * l of tests/test_proxnpi_kernel_gpu.py and of the plugin tests (16 x 16: two rows, four rows)
KERNEL_N = (256, 512, 3200, 23232, 32768, 73728, 147456, 2048, 4096)


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


@pytest.mark.parametrize("shape,kind", GUIDANCE_CASES)
def test_guidance_vs_reference(golden, shape, kind):
    g = golden("proxnpi_guidance")
    u, c = pr.guidance_inputs(shape, kind, pr.guidance_seed(shape, kind))
    np.testing.assert_array_equal(np.concatenate([u.ravel()[:4], c.ravel()[:4]]), g[f"probe/{'x'.join(map(str, shape))}/{kind}"])
    if kind == "zero_row":
        assert not (c[0] - u[0]).any() and (c[1:] - u[1:]).any()
    if kind == "eighths":
        assert not ((c - u) * 8 % 1).any()
    keep = guidance_keep(shape)
    worst64 = worst32 = 0.0
    for prox, q in GUIDANCE_SETTINGS:
        want64, want32 = g[guidance_key(shape, kind, prox, q, "f64")], g[guidance_key(shape, kind, prox, q, "f32")]
        assert want64.dtype == np.float64 and want32.dtype == np.float32
        got64, _ = pr.guidance(u, c, GUIDANCE_G, prox, q, np.float64)
        e64 = np.abs(got64.ravel()[keep] - want64).max()
        worst64 = max(worst64, e64)
        assert e64 <= 1e-12, (prox, q, e64)
        # float32: the same operations in the same order on the same fp32 inputs.  d = c - u and the sort are exact, the rank split is the same
        # fp32 product; what may differ is contraction inside torch's lerp (the threshold: one ulp of it), which the shrinkage passes on to d'
        # (one ulp of thr, times g) and the final sum rounds once more (half an ulp of the result)
        got32, thr = pr.guidance(u, c, GUIDANCE_G, prox, q, np.float32)
        assert got32.dtype == np.float32
        bound = (GUIDANCE_G * ulp32(thr) if thr is not None else 0.0) + 0.5 * ulp32(np.abs(want32).max())
        e32 = np.abs(got32.ravel()[keep].astype(np.float64) - want32).max()
        worst32 = max(worst32, e32 / bound)
        assert e32 <= bound, (prox, q, e32, bound)
    print(f"{shape} {kind}: float64 restatement within {worst64:.3e} of the reference; float32 at {worst32:.2f} of its bound")


def test_settings_differ(golden):
    """the fixture separates its settings: l0 from l1, every quantile from the next, and quantile 0 from plain CFG by nothing"""
    g = golden("proxnpi_guidance")
    shape, kind = (2, 4, 20, 20), "white"
    get = lambda prox, q: g[guidance_key(shape, kind, prox, q, "f64")]
    assert np.abs(get("l0", 0.7) - get("l1", 0.7)).max() > 1e-2 and np.abs(get("l0", 0.7) - get("l0", 0.3)).max() > 1e-2
    assert np.abs(get("l0", 1.0) - get("l0", 0.7)).max() > 1e-2 and np.abs(get("l0", -0.25) - get("l0", 0)).max() > 1e-2
    np.testing.assert_array_equal(get("l0", 0), get(None, 0.7))
    u, c = pr.guidance_inputs(shape, kind, pr.guidance_seed(shape, kind))
    np.testing.assert_array_equal(get("l0", 1.0), u.astype(np.float64).ravel()[guidance_keep(shape)])      # the largest |d| as threshold: nothing passes


def test_rank_split_matches_torch_quantile():
    from etainv.pipeline import ProximalGuidance
    rng = np.random.default_rng(11)
    gen = torch.Generator().manual_seed(11)
    cases = [(n, q) for n in KERNEL_N for q in (0.7, 0.3, 1.0, 1e-6, 0.5)]
    cases += [(int(rng.integers(1, 5000)), float(rng.random())) for _ in range(200)] + [(1, 0.7), (2, 1.0), (2, 0.5)]
    for i, (n, q) in enumerate(cases):
        x = torch.randn(n, generator=gen).abs()
        if i % 3 == 1:
            x = torch.round(x * 4) / 4                                              # heavy ties
        k, w = pr.rank_split(n, q)
        assert (k, float(w)) == ProximalGuidance.rank_split(n, q), (n, q)
        assert 0 <= k <= n - 1 and 0.0 <= w < 1.0
        s = torch.sort(x).values
        got = torch.lerp(s[k], s[min(k + 1, n - 1)], torch.tensor(float(w)))
        assert got.item() == torch.quantile(x, q).item(), (n, q, k, float(w))
        # and the restatement's own threshold (numpy float32) is that value to the contraction inside torch's lerp
        thr, lo, hi = pr.threshold(x.numpy(), q, np.float32)
        assert lo == s[k].item() and hi == s[min(k + 1, n - 1)].item() and abs(float(thr) - got.item()) <= ulp32(hi)
    assert pr.rank_split(32768, 1.0) == (32767, 0.0) and pr.rank_split(2048, 0.7)[0] == 1432


def test_l1_rule_table():
    """the reference's three lines (:88-90) with thr = 1: not symmetric, jumps at d = -thr and d = 2 thr"""
    d = np.array([-3.0, -1.5, 1.5, 2.0, 3.0, 0.5, -0.5, 1.0, -1.0])
    np.testing.assert_array_equal(pr.shrink(d, 1.0, "l1"), [-1.0, 0.5, 0.5, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0])
    np.testing.assert_array_equal(pr.shrink(d, 1.0, "l0"), [-2.0, -0.5, 0.5, 1.0, 2.0, 0.0, 0.0, 0.0, 0.0])
    t = torch.from_numpy(d)
    s = t - t.clamp(-1.0, 1.0)
    s = torch.where(s > 0, s - 1.0, s)
    s = torch.where(s < 0, s + 1.0, s)
    np.testing.assert_array_equal(pr.shrink(d, 1.0, "l1"), s.numpy())
    eps = 1e-9
    assert pr.shrink(np.array([-1.0 - eps]), 1.0, "l1")[0] > 0.99 and pr.shrink(np.array([-1.0 + eps]), 1.0, "l1")[0] == 0.0
    assert pr.shrink(np.array([2.0 - eps]), 1.0, "l1")[0] > 0.99 and pr.shrink(np.array([2.0 + eps]), 1.0, "l1")[0] < 1e-8
    with pytest.raises(NotImplementedError):
        pr.shrink(d, 1.0, "l2")


@pytest.mark.parametrize("l", [8, 16, 20, 64])
def test_half_zero_consequence(l):
    """over [a row whose d is zero, the target row] the zeros fill the low ranks: the threshold at q = 0.7 is the target row's own order
    statistics at the rank the split gives minus the number of zeros -- about its 0.4-quantile"""
    gen = torch.Generator().manual_seed(l)
    tgt = torch.randn(4 * l * l, generator=gen).numpy()
    d = np.stack([np.zeros_like(tgt), tgt])
    n = d.size
    k, w = pr.rank_split(n, 0.7)
    assert k >= n // 2
    s = np.sort(np.abs(tgt))
    thr, lo, hi = pr.threshold(d, 0.7, np.float32)
    assert lo == s[k - n // 2] and hi == s[k + 1 - n // 2] and thr == pr.lerp(lo, hi, w)
    assert thr == np.float32(torch.quantile(torch.from_numpy(d).abs().flatten(), 0.7).item())
    q_own = (k - n // 2 + float(w)) / (n // 2 - 1)
    assert abs(q_own - 0.4) < 2.0 / (n // 2)
    assert abs(float(thr) - torch.quantile(torch.from_numpy(np.abs(tgt)), q_own).item()) <= 4 * ulp32(hi)


@pytest.mark.parametrize("tag", list(VARIANTS))
def test_loop_vs_reference(golden, tag):
    """NpiRef over the toy oracle UNet vs the reference's `invert` and `sample([source, target])` (fp32 there), at the bounds
    tests/test_oracle_golden.py holds e2e_diffinv to: the inversion (guidance 1) and the edited latents (guidance 7.5)"""
    from oracle.unet import build_unet
    from tests.edict_ref import torch_unet
    g, d = golden("e2e_npi"), golden("e2e_diffinv")
    ctx_s, ctx_t = d["ctx_src"], d["ctx_tgt"]
    np.testing.assert_array_equal(np.concatenate([ctx_s.ravel()[:4], ctx_t.ravel()[-4:]]), g["ctx_probe"])
    assert int(g["S"]) == E2E_S and g["z0"].shape == (1, 4, E2E_L, E2E_L)
    toy = torch_unet(build_unet(0, block_out_channels=(32, 64, 128, 128)))
    ref = pr.NpiRef(toy, E2E_S, prox=VARIANTS[tag])
    lat = ref.invert(g["z0"], ctx_s)
    np.testing.assert_allclose(lat[:, 0], g[f"{tag}/inv_latents"], rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(g[f"{tag}/inv_latents"], g["npi/inv_latents"], rtol=1e-4, atol=2e-5)   # the inversion is the base class's in all three
    edit, thrs, ds = ref.sample(lat[-1], ctx_s, [ctx_s, ctx_t])
    np.testing.assert_allclose(edit, g[f"{tag}/edit"], rtol=1e-3, atol=2e-4)
    if VARIANTS[tag] is not None:
        assert all(np.abs(x[0]).max() <= 1e-6 * np.abs(x[1]).max() for x in ds)            # the source pair's d: zero, or a rounding's worth
        assert np.abs(edit - pr.NpiRef(toy, E2E_S).sample(lat[-1], ctx_s, [ctx_s, ctx_t])[0]).max() > 1e-2      # the threshold is not a no-op
