"""CPU checks of tests/attention_ref.py: the helpers the GPU attention tests rest on, and the condition that makes their per-item bounds legitimate
(an ideal 16-bit flash kernel -- emulate_16bit -- uses at most half of every bound on every input family those tests run)."""
import itertools
import math
import pathlib
import subprocess

import pytest
import torch

from tests import attention_ref as AR

DTYPES = [torch.float16, torch.bfloat16]


def test_layout_round_trip():
    b, n, heads, d = 3, 64, 4, 40
    qkv = AR.random_qkv(b, n, heads, d, torch.float16, 0)
    planes = AR.to_head_major(qkv, heads)
    assert planes.shape == (3, b, heads, n, d) and planes.is_contiguous()
    assert torch.equal(AR.from_head_major(planes, b, n, heads), qkv)
    assert torch.equal(AR.from_head_major(planes.reshape(-1), b, n, heads), qkv)        # (a flat device buffer)
    # element by element: plane p, row r, head h, token t, dim j  <-  qkv[r, t, p * C + h * d + j]
    for p, r, h, t, j in [(0, 0, 0, 0, 0), (1, 2, 3, 63, 39), (2, 1, 2, 17, 5)]:
        assert planes[p, r, h, t, j] == qkv[r, t, p * heads * d + h * d + j]


def _brute_force_four_row(n_img, mode):
    """(q, k, v) source rows of the four-row call, image by image, from the words of the two papers' code: rows [u_s, u_t, c_s, c_t] x n_img."""
    src = {}
    for img in range(n_img):
        u_s, u_t, c_s, c_t = (role * n_img + img for role in range(4))
        for r in (u_s, u_t, c_s, c_t):
            src[r] = [r, r, r]
        if mode == 1:
            src[c_t][0] = src[c_t][1] = c_s
        if mode == 2:
            src[u_t][1] = src[u_t][2] = u_s
            src[c_t][1] = src[c_t][2] = c_s
    return src


@pytest.mark.parametrize("n_img", [1, 2, 8])
def test_row_maps_against_enumeration(n_img):
    for mode in (0, 1, 2):
        qm, km, vm = AR.row_maps(4 * n_img, n_img, mode, 0)
        src = _brute_force_four_row(n_img, mode)
        for r in range(4 * n_img):
            assert [int(qm[r]), int(km[r]), int(vm[r])] == src[r], (mode, r)
    # the three-row forms select the same source ROWS OF THE FOUR-ROW TENSOR
    src = _brute_force_four_row(n_img, 1)
    for first_row in (n_img, -1):
        qm, km, vm = AR.row_maps(3 * n_img, n_img, 1, first_row)
        in4 = AR.rows_in_four_row_call(n_img, first_row)
        assert sorted(in4.tolist()) == list(range(n_img, 4 * n_img))
        for r in range(3 * n_img):
            assert [int(in4[qm[r]]), int(in4[km[r]]), int(in4[vm[r]])] == src[int(in4[r])], (first_row, r)
    with pytest.raises(AssertionError):
        AR.row_maps(3 * n_img, n_img, 2, n_img)


def test_row_maps_three_row_reference_equals_rows_of_the_four_row_reference():
    n_img, n, heads, d = 2, 64, 2, 40
    qkv4 = AR.random_qkv(4 * n_img, n, heads, d, torch.float16, 3)
    ref4 = AR.ref_self_attention(qkv4, heads, *AR.row_maps(4 * n_img, n_img, 1, 0))
    for first_row in (n_img, -1):
        in4 = AR.rows_in_four_row_call(n_img, first_row)
        ref3 = AR.ref_self_attention(qkv4[in4], heads, *AR.row_maps(3 * n_img, n_img, 1, first_row))
        assert torch.equal(ref3, ref4[in4])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [40, 80])
def test_prescaled_reference_equals_plain_reference_on_the_same_queries(dtype, d):
    """q' carries scale * log2 e exactly when the product needs no rounding: take q' first, then q := q' / (scale log2 e) in float64."""
    b, n, heads = 1, 128, 2
    qkv = AR.prescale_q(AR.random_qkv(b, n, heads, d, dtype, 5), heads, d)            # q' representable in dtype
    plain = qkv.double()
    plain[..., : heads * d] /= d ** -0.5 * AR.LOG2E                                    # the real-valued q it stands for
    a = AR.ref_self_attention(qkv, heads, prescaled=True, dt=torch.float64)
    r = AR.ref_self_attention(plain, heads, dt=torch.float64)
    assert ((a - r).norm() / r.norm()).item() < 1e-12
    # and prescale_q itself: within half an ulp of the operand type of the exact product
    x = AR.random_qkv(b, n, heads, d, dtype, 6)
    q1 = AR.prescale_q(x, heads, d)[..., : heads * d].double()
    q0 = x[..., : heads * d].double() * (d ** -0.5 * AR.LOG2E)
    eps = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
    assert ((q1 - q0).abs() <= eps * q0.abs() * 1.001 + 1e-7).all()
    assert torch.equal(AR.prescale_q(x, heads, d)[..., heads * d:], x[..., heads * d:])


def test_attn_errors_finds_one_wrong_block_and_one_wrong_query():
    b, n, heads, d = 2, 256, 4, 40
    ref = torch.randn(b, n, heads * d, generator=torch.Generator().manual_seed(0))
    out = ref.clone()
    out[1, 96:128, 2 * d:3 * d] *= 1.3                     # block 3 of (row 1, head 2) wrong by 30 %
    g, blk, qry, where = AR.attn_errors(out, ref, heads, d)
    assert where["block"] == dict(row=1, head=2, block=3) and abs(blk - 0.3) < 1e-6
    assert g < 0.3 / math.sqrt(b * heads * n / 32) * 1.5
    out = ref.clone()
    out[0, 200, 1 * d:2 * d] = 0                           # one query entirely wrong
    g, blk, qry, where = AR.attn_errors(out, ref, heads, d)
    assert where["query"] == dict(row=0, head=1, query=200) and abs(qry - 1.0) < 1e-6
    assert where["block"] == dict(row=0, head=1, block=6)
    # ragged token counts: the last block holds n % 32 queries
    out = ref.clone()
    out[1, 195, 3 * d:] *= 1.5
    g, blk, qry, where = AR.attn_errors(out[:, :200], ref[:, :200], heads, d)
    assert where["block"] == dict(row=1, head=3, block=6) and where["query"] == dict(row=1, head=3, query=195)
    assert abs(qry - 0.5) < 1e-6 and 0.5 / math.sqrt(8) * 0.5 < blk < 0.5


# (dtype-independent) input families of the GPU tests: (N, d, gain) -> the tolerance factor their test applies
FAMILIES = {
    # test_self_attention_plain
    (4096, 40, 1.0): 1, (1024, 80, 1.0): 1, (256, 160, 1.0): 1, (64, 160, 1.0): 1, (144, 160, 1.0): 1, (576, 80, 1.0): 1,
    # test_self_attention_d40 / d80 / d160
    (256, 40, 1.0): 1, (64, 40, 1.0): 1, (144, 40, 1.0): 1, (200, 40, 1.0): 1, (576, 40, 1.0): 1, (1024, 40, 3.0): 2, (2304, 40, 0.05): 1, (9216, 40, 1.0): 1,
    (256, 80, 1.0): 1, (144, 80, 1.0): 1, (200, 80, 1.0): 1, (1024, 80, 3.0): 2, (2304, 80, 0.05): 1,
    (200, 160, 3.0): 2, (1024, 160, 0.05): 1,
    # the persistent-kernel tests, the remap tests and tests/test_attention_forms_gpu.py
    (2048, 40, 1.0): 1, (1024, 40, 1.0): 1, (2304, 80, 1.0): 1, (320, 40, 1.0): 1,
}


@pytest.mark.parametrize("dtype", DTYPES)
def test_emulation_stays_below_half_of_every_bound(dtype):
    """The legitimacy of the per-block / per-query bounds: rounding P and the output alone (fp32 sums, exact maximum) costs at most 0.5 x each bound on every
    family, plain and pre-scaled.  heads = 2, b = 1 (one head at N = 9216)."""
    worst = [0.0, 0.0, 0.0]
    for (n, d, gain), factor in FAMILIES.items():
        heads = 1 if n > 4096 else 2
        qkv = AR.random_qkv(1, n, heads, d, dtype, n + d, gain)
        forms = [(qkv, False)]
        if d <= 80 and n >= 1024:
            forms.append((AR.prescale_q(qkv, heads, d), True))      # the engine's form (only the larger launches are tested in it)
        for x, pre in forms:
            ref = AR.ref_self_attention(x, heads, prescaled=pre, dt=torch.float64)
            errs = AR.attn_errors(AR.emulate_16bit(x, heads, prescaled=pre), ref, heads, d)[:3]
            for i, (e, bnd) in enumerate(zip(errs, AR.bounds(dtype, factor))):
                worst[i] = max(worst[i], e / bnd)
                assert e <= 0.5 * bnd, (n, d, gain, pre, i, e, bnd)
    print(f"emulation / bound, worst over the families: global {worst[0]:.2f} block {worst[1]:.2f} query {worst[2]:.2f}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_emulation_on_the_adversarial_inputs(dtype):
    """The inputs of ..._speculative_maximum (4 rows) and ..._exact_pass (16 rows), bounds x 1.5 as in those tests: every row, the boosted ones included, stays
    below half of the per-item bounds under the emulation (exact maximum), so the GPU tests apply them to every row."""
    heads, n, d = 8, 2048, 40
    for name, b, seed, items in (("speculative_maximum", 4, 123, AR.SPECULATIVE_ITEMS), ("exact_pass", 16, 321, AR.EXACT_PASS_ITEMS)):
        qkv = AR.speculative_maximum_qkv(b, heads, n, d, dtype, seed, items)
        rows = sorted({0, 1, 2, 3} | {it[0] for it in items})                      # (the other rows of the 16-row input are plain random rows like row 0)
        x = qkv[rows]
        ref = AR.ref_self_attention(x, heads, dt=torch.float64)
        errs = AR.attn_errors(AR.emulate_16bit(x, heads), ref, heads, d)[:3]
        for e, bnd in zip(errs, AR.bounds(dtype, 1.5)):
            assert e <= 0.5 * bnd, (name, e, bnd)


def test_emulation_on_maximum_jumps_late():
    qkv = AR.maximum_jumps_late_qkv()
    ref = AR.ref_self_attention(qkv, 8, dt=torch.float64)
    errs = AR.attn_errors(AR.emulate_16bit(qkv, 8), ref, 8, 40)[:3]
    for e, bnd in zip(errs, AR.bounds(torch.float16)):
        assert e <= 0.5 * bnd, (e, bnd)


def test_scaled_query_rounding_on_maximum_jumps_late():
    """Why that test takes its single-query bound against the reference of the rounded scaled queries: rounding q d^-0.5 log2 e to fp16 -- the MFMA's operand type,
    done by the kernel when q_prescaled = 0 and by the to_q projection in the engine -- alone moves single queries of this input by more than 2 x TOL, with EXACT
    attention behind it; against the reference of the rounded queries the emulation is back below half of every bound."""
    heads, d, dtype = 8, 40, torch.float16
    qkv = AR.maximum_jumps_late_qkv(dtype)
    exact = AR.ref_self_attention(qkv, heads, dt=torch.float64)
    rounded = AR.prescale_q(qkv, heads, d)
    exact_on_rounded = AR.ref_self_attention(rounded, heads, prescaled=True, dt=torch.float64)
    g, blk, qry, where = AR.attn_errors(exact_on_rounded, exact, heads, d)
    bg, bb, bq = AR.bounds(dtype)
    assert g < 0.5 * bg and blk < 0.5 * bb          # global and per block the rounding stays small ...
    assert qry > bq, qry                             # ... a single query does not (4.5e-3 against 4e-3)
    errs = AR.attn_errors(AR.emulate_16bit(rounded, heads, prescaled=True), exact_on_rounded, heads, d)[:3]
    for e, bnd in zip(errs, (bg, bb, bq)):
        assert e <= 0.5 * bnd, (e, bnd)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,n", [(40, 2048), (80, 1024)])
def test_coded_inputs_decode_to_the_row_maps(dtype, d, n):
    """With the fp32 reference and row_maps alone the decoded ids are the expected ones -- in every layout, plain and pre-scaled; the peak owns the softmax."""
    n_img, heads = 8, 2
    for mode, first_row in [(0, 0), (1, 0), (2, 0), (1, n_img), (1, -1)]:
        b = 3 * n_img if first_row else 4 * n_img
        maps = AR.row_maps(b, n_img, mode, first_row)
        for pre in (False, True):
            x = AR.coded_qk_qkv(b, n, heads, d, dtype)
            x = AR.prescale_q(x, heads, d) if pre else x
            q = x[0, 0, :d].double().abs().max() * x[0, :, heads * d: heads * d + d].double().abs().max()
            assert q * (math.log(2.0) if pre else d ** -0.5) >= 30.0
            ref = AR.ref_self_attention(x, heads, *maps, prescaled=pre)
            assert torch.equal(AR.decode_tokens(ref, heads, d), AR.expected_tokens(maps[0], maps[1], n, heads))
        x = AR.coded_v_qkv(b, n // 8, heads, d, dtype, 11)
        ref = AR.ref_self_attention(x, heads, *maps)
        assert torch.equal(AR.decode_v_ids(ref, heads, d), AR.expected_v_ids(maps[2], n // 8, heads))
    # the codes tell rows apart: a wrong map is seen
    maps = AR.row_maps(4 * n_img, n_img, 1, 0)
    x = AR.coded_qk_qkv(4 * n_img, n, heads, d, dtype)
    wrong = AR.ref_self_attention(x, heads, maps[0], torch.arange(4 * n_img), maps[2])
    assert not torch.equal(AR.decode_tokens(wrong, heads, d), AR.expected_tokens(maps[0], maps[1], n, heads))


# every (b, n, heads, d) that tests/test_kernels_gpu.py and tests/test_attention_forms_gpu.py launch on the 16-bit self-attention kernels
LAUNCHED = sorted({
    # test_kernels_gpu.py: plain
    (2, 4096, 8, 40), (2, 1024, 8, 80), (2, 256, 8, 160), (2, 64, 8, 160), (2, 144, 8, 160), (2, 576, 8, 80),
    # ... d40 / d80 / d160
    (2, 256, 8, 40), (1, 64, 8, 40), (1, 144, 4, 40), (3, 200, 4, 40), (1, 576, 8, 40), (2, 1024, 8, 40), (1, 2304, 8, 40), (1, 9216, 8, 40),
    (2, 256, 8, 80), (1, 144, 4, 80), (3, 200, 4, 80), (2, 1024, 8, 80), (1, 2304, 8, 80),
    (4, 256, 8, 160), (2, 64, 8, 160), (1, 144, 4, 160), (3, 200, 4, 160), (1, 1024, 8, 160), (8, 256, 8, 160),
    # ... maximum_jumps_late, single_row, speculative_maximum, the persistent-kernel tests, the remap tests, the MasaCtrl golden
    (1, 512, 8, 40), (16, 4096, 8, 40), (1, 4096, 8, 40), (4, 2048, 8, 40),
    (16, 2048, 8, 40), (33, 1024, 8, 40), (33, 2048, 4, 40), (9, 4096, 8, 40),
    (16, 1024, 8, 80), (8, 2304, 8, 80), (33, 1024, 4, 80),
    (8, 320, 8, 40), (8, 256, 8, 80), (4, 64, 8, 40),
    # test_attention_forms_gpu.py: engine form, config 5, row layouts / item decoder (32 and 24 rows), rejected forms, projection planes, largest tensor
    (4, 4096, 8, 40), (4, 1024, 8, 80), (16, 1024, 8, 80), (8, 9216, 8, 40), (16, 9216, 8, 40), (11, 2304, 8, 80),
    (32, 1024, 8, 80), (24, 1024, 8, 80), (32, 2048, 8, 40), (24, 2048, 8, 40),
    (6, 256, 8, 80), (2, 256, 8, 40),
    (546, 4096, 8, 40), (547, 4096, 8, 40),
})

ROUTE_DRIVER = """
#include <stdio.h>
#include "self_attn_route.h"
int main() {
  int b, n, heads, d, n_cu, p40, p80;
  while (scanf("%d %d %d %d %d %d %d", &b, &n, &heads, &d, &n_cu, &p40, &p80) == 7) printf("%d\\n", (int)etainv::self_attn_route(b, n, heads, d, n_cu, p40, p80));
}
"""


def test_route_mirror_equals_the_launcher_rule(tmp_path):
    """AR.self_attention_route against self_attn_route of csrc/self_attn_route.h (the function launch_self_attention_mode switches on), compiled with the host
    compiler: every launched shape, 8 / 256 / 304 CUs, both settings of the two persist switches."""
    csrc = pathlib.Path(__file__).resolve().parents[1] / "eta-inversion_amd" / "csrc"
    (tmp_path / "driver.cpp").write_text(ROUTE_DRIVER)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", str(csrc), "-o", str(tmp_path / "driver"), str(tmp_path / "driver.cpp")], check=True)
    cases = [(*shape, n_cu, p40, p80) for shape in LAUNCHED for n_cu in (8, 256, 304) for p40, p80 in itertools.product((1, 0), repeat=2)]
    out = subprocess.run([str(tmp_path / "driver")], input="".join(" ".join(map(str, c)) + "\n" for c in cases), capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == len(cases)
    seen = set()
    for (b, n, heads, d, n_cu, p40, p80), got in zip(cases, out):
        want = AR.self_attention_route(b, n, heads, d, n_cu, bool(p40), bool(p80))
        assert AR.ROUTES[int(got)] == want, (b, n, heads, d, n_cu, p40, p80)
        seen.add(want)
    assert seen == set(AR.ROUTES)          # the cases reach all six routes
