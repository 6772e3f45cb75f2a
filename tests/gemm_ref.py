"""Plain-PyTorch references for every route of launch_igemm (csrc/igemm.hip, csrc/ppgemm.hip, csrc/ppconv.hip, the fp32 twin in csrc/f32path.hip) -- no GPU
needed, no import of the library.  Device-agnostic torch in the style of tests/norm_ref.py: tests/test_gemm_ref.py runs it on the CPU, tests/test_gemm_routes_gpu.py
on the device (float64 matmul there too), on the SAME operands, which the case list at the end of this module defines.

  references   float64, from the rounded operands the kernel reads.  Every launch is `acc = A W^T` with A the activation rows: the rows themselves for a Linear /
               1x1 (second source: concatenated channels), explicitly gathered taps for a conv3x3 (tap_index: pad 1, stride 1 / 2, pad0, the nine taps on the
               nearest-2x grid; the four-phase form gathers 2 x 2 taps per phase against the packed phase weights, pack_ups4_ref).  Then the epilogue: bias
               (per image for per-image weights), time row per image, residual; the folded-LayerNorm consumer rstd (acc - mean s) + c on the `stat` rows it is
               given; GEGLU a gelu(g) with float64 erf on the pack-mode-2 column order (geglu_split); hm_index maps [M][N] to the head-major planes.
  bounds       per element, counted, no tuned constant (u = 2^-24):
                 e = gamma_l(K_total + ksplit + 4) (sum_k |a||w| + |bias| + |rowvec| + |residual|),      bound = U_RND (|ref| + e) + e + ABS_FLOOR
               exact 16-bit products, an fp32 chain of K_total additions, one addition per K part of a split, the epilogue's additions (the form of
               norm_ref.gemm_ln_bound).  fp32 operands: the same e (a product rounds once where the 16-bit product is exact; the 4 spare cover it), U_RND = 0.
               LayerNorm consumer: e = gamma_l(.) (|rstd| (sum |a||w| + |mean s|) + |c|).
               GEGLU: out = a gelu(g) with |a' - a| <= e_a, |g' - g| <= e_g:  e_gelu = GELU_LIP e_g + |g| / 2 ERF_ERR + 2 u |gelu(g)|  (h = g / 2 is exact, h s + h
               one fma; ERF_ERR below),  e = |a| e_gelu + |gelu(g)| e_a + e_a e_gelu + u |a gelu(g)|.
               LayerNorm-producer partials (mean, M2) of a row's 80-column chunk against float64 statistics of the STORED row (ln_partial_err), GroupNorm-producer
               partials (sum, sum of squares per channel over 64 stored rows) by a chain of 64 (gn_partial_err).
  emulation    the best fp32 can do: fp32 matmul of the same operands, the epilogue in fp32 in the kernel's order, returned BEFORE the output rounding (the
               convention of norm_ref: a condition |emulation - ref| <= e / 2 on the part of the bound in front of the rounding).  `fault` breaks it one way at
               a time, which tests/test_gemm_ref.py uses to show that both families can fail.
  families     random: a ~ N(0, 1), w ~ N(0, 1 / K), bias ~ N(0.5, 1), residual ~ N(0, 2^2), a time row per image with distinct image means, stat rows with
               means well off zero and rstd varying 4x from row to row.  exact: every operand a small integer given by a hash of its indices (a, w in
               {-1, 0, 1}, bias and time row in [-8, 8], residual in [-16, 16], stat = (integer mean, power-of-two rstd), s and c integers): every product and
               every fp32 partial sum is an integer, the stored value is representable, and the kernel must equal the reference bit for bit in any order.
               The density of w falls with K (96 / K non-zeros from K = 144 on) so that |ref| stays far below 256, the largest range in which bf16 holds
               every integer; tests/test_gemm_ref.py asserts max |ref| <= 256, representability and that neighbouring rows, columns, images, taps and K tiles
               of every operand differ.

ERF_ERR.  gelu_pair_emu restates gelu_pair of csrc/common.h operation by operation in fp32 (torch.exp2 for the hardware exp2).  measure_erf_error evaluates its
erf against float64 erf on 1,200,001 fp32 points over [-6, 6]: 1.721e-7 (ERF_MEASURED; csrc/common.h claims 1.8e-7 -- the claim holds).  The bound adds 2 fp32 ulp
(2 x 2^-23, of a value <= 1) for the hardware exp2.  GELU_LIP = 1.13: the maximum of |gelu'| is 1.1290 at g = 1.414."""
import functools
import math
import types
import zlib

import torch

from tests.norm_ref import ABS_FLOOR, DTYPES16, DTYPES3, NAME, U32, U_RND, gamma_l, worst  # noqa: F401  (re-exported to the tests)

GELU_LIP = 1.13
ERF_MEASURED = 1.721e-7
ERF_ERR = ERF_MEASURED + 2 * 2.0 ** -23
FAMILIES = ["random", "exact"]
ROUTES = ["ppconv", "dualn", "ring-ups4", "ring-ups9", "ring-patch", "ring", "ring-geglu", "two-slot", "fp32"]      # kIGemmRouteName of csrc/igemm.hip
TIME_COLUMNS, TIME_OFFSET = 20160, 6720        # the UNet's matrix of all time projections, and a layer's column block inside it


# ---------------------------------------------------------------------------------------------------------------- layouts
def geglu_split(h):
    """[m][N] in the pack-mode-2 (physical) column order -> (value, gate), each [m][N / 2] in output order: block q of 64 physical columns holds the
    value columns 32 q .. 32 q + 31 and their gates"""
    v = h.reshape(h.shape[0], -1, 2, 32)
    return v[:, :, 0].reshape(h.shape[0], -1), v[:, :, 1].reshape(h.shape[0], -1)


def pack_geglu(w):
    """row interleave used by the GEGLU epilogue (csrc/misc.hip pack mode 2): logical rows [value | gate] -> physical rows"""
    rows = w.shape[0]
    p = torch.arange(rows)
    blk, within = p // 64, p % 64
    logical = torch.where(within < 32, blk * 32 + within, rows // 2 + blk * 32 + within - 32)
    return w[logical]


def hm_index(m, n, heads, dim, tokens, device="cpu"):
    """flat index into the planes [q|k|v][row][head][token][dim] of the element (row m, column n) of the row-major [M][N] result; rows = M / tokens"""
    mm, nn = torch.arange(m, device=device)[:, None], torch.arange(n, device=device)[None, :]
    part, head, d = nn // (heads * dim), nn // dim % heads, nn % dim
    return (((part * (m // tokens) + mm // tokens) * heads + head) * tokens + mm % tokens) * dim + d


def tap_index(h, w, ho, wo, stride, pad, ups, taps, shift_tap=None):
    """[Ho Wo][taps] indices into the H W source pixels of an image, H W where the tap reads the zero padding.  taps: (dy, dx) per tap.  ups: the taps move on
    the nearest-2x grid.  shift_tap (a fault): tap 0 of the first output row reads one pixel further down instead of the padding"""
    oy, ox = torch.arange(ho)[:, None, None], torch.arange(wo)[None, :, None]
    dy, dx = torch.tensor([t[0] for t in taps])[None, None, :], torch.tensor([t[1] for t in taps])[None, None, :]
    sy, sx = oy * stride + dy - pad, ox * stride + dx - pad
    if shift_tap is not None:
        sy = torch.where((oy == 0) & (torch.arange(len(taps))[None, None, :] == shift_tap), sy + 1, sy)
    if ups:
        ok = (sy >= 0) & (sy < 2 * h) & (sx >= 0) & (sx < 2 * w)
        sy, sx = sy.clamp(min=0) // 2, sx.clamp(min=0) // 2
    else:
        ok = (sy >= 0) & (sy < h) & (sx >= 0) & (sx < w)
    return torch.where(ok, sy * w + sx, torch.full_like(sy + sx, h * w)).reshape(ho * wo, len(taps))


TAPS9 = [(ky, kx) for ky in range(3) for kx in range(3)]


def phase_taps(py, px):
    """the 2 x 2 source taps of output phase (py, px) of conv3x3(nearest-2x upsample): tap (ty, tx) reads source pixel (sy + ty - 1 + py, sx + tx - 1 + px)"""
    return [(ty + py, tx + px) for ty in range(2) for tx in range(2)]


def pack_ups4_ref(w_oc33, dtype):
    """what etainv_op_pack_ups4 leaves: [phase py px][cout][tap ty tx][cin], each the fp32 sum (ky outer, kx inner, from zero) of the 3 x 3 taps that share a
    source pixel, rounded once.  float64 in -> the exact sums, not rounded (dtype None)"""
    cout, cin = w_oc33.shape[:2]
    out = torch.zeros(4, cout, 4, cin, dtype=w_oc33.dtype, device=w_oc33.device)
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    kys = ([0], [1, 2]) if py == 0 else ([0, 1], [2])
                    kxs = ([0], [1, 2]) if px == 0 else ([0, 1], [2])
                    v = torch.zeros(cout, cin, dtype=w_oc33.dtype, device=w_oc33.device)
                    for ky in kys[ty]:
                        for kx in kxs[tx]:
                            v = v + w_oc33[:, :, ky, kx]
                    out[py * 2 + px, :, ty * 2 + tx] = v
    return out if dtype is None else out.to(dtype)


# ---------------------------------------------------------------------------------------------------------------- GELU
def gelu64(g):
    g = g.double()
    return 0.5 * g * (1.0 + torch.erf(g * 0.7071067811865476))


def _f(v):
    return torch.tensor(v, dtype=torch.float32)


def erf_emu(x):
    """copysign(1 - exp2(-p(min(|x| / sqrt 2, 4.3))), x) as gelu_pair (csrc/common.h) evaluates it: fp32, every product-and-sum one fma"""
    x = x.float()

    def fma(a, b, c):
        return (a.double() * b.double() + c.double()).float()
    ax = torch.minimum(x.abs() * _f(0.70710678118654752), _f(4.3))
    p = fma(ax, _f(0.000100211372), _f(-0.000461519738))
    for c in (-0.00230234699, 0.0294526188, -0.148963716, -0.918328635, -1.62791373):
        p = fma(p, ax, _f(c))
    er = 1.0 - torch.exp2(p * ax)
    return torch.copysign(er, x)


def gelu_pair_emu(x):
    x = x.float()
    h = x * 0.5
    return (h.double() * erf_emu(x).double() + h.double()).float()


def measure_erf_error(lo=-6.0, hi=6.0, n=1200001):
    """worst |erf_emu(x) - erf64(x / sqrt 2)| over fp32 x on a dense grid"""
    x = torch.linspace(lo, hi, n, dtype=torch.float64).float()
    return float((erf_emu(x).double() - torch.erf(x.double() * 0.7071067811865476)).abs().max())


# ---------------------------------------------------------------------------------------------------------------- the cases
class Case:
    """one launch: the shape, what the epilogue does and the plan launch_igemm must report.  kind "lin": a [m][k1] (+ a2 [m][k2]); kind "conv": a
    [b][h][w][k1] NHWC (+ a2), w [n][taps][k1 + k2]; ups 1 = nine taps on the upsampled grid, 2 = the four-phase form.  `images` > 1 with kind "lin": the rows
    are `images` images of m / images rows (time row, GroupNorm partials, per-image weights)"""

    def __init__(self, name, kind, plan, entry, m=0, n=0, k1=0, k2=0, images=1, h=1, w=1, stride=1, ups=0, pad0=0, bias=True, time=False, time_strided=False,
                 res=False, ln=False, geglu=False, hm=0, f32out=False, lnprod=False, gnprod=False, per_image=False, fp32_too=False):
        self.name, self.kind, self.entry = name, kind, entry
        self.plan = dict(zip(("route", "bm", "bn", "ksplit", "form"), plan))
        self.n, self.k1, self.k2, self.images, self.h, self.w, self.stride, self.ups, self.pad0 = n, k1, k2, images, h, w, stride, ups, pad0
        self.bias, self.time, self.time_strided, self.res, self.ln, self.geglu, self.hm = bias, time, time_strided, res, ln, geglu, hm
        self.f32out, self.lnprod, self.gnprod, self.per_image, self.fp32_too = f32out, lnprod, gnprod, per_image, fp32_too
        if kind == "conv":
            self.ho, self.wo = (2 * h, 2 * w) if ups else (h // 2, w // 2) if stride == 2 else (h, w)
            self.taps = 4 if ups == 2 else 9
            self.m = images * self.ho * self.wo
            self.rows_per_image = self.ho * self.wo
        else:
            self.ho, self.wo, self.taps, self.m = 1, 1, 1, m
            self.rows_per_image = m // images
        self.k_total = self.taps * (k1 + k2)
        self.n_out = n // 2 if geglu else n
        self.shape_key = (kind, self.m, n, k1, k2, images, h, w, stride, ups, pad0, per_image)

    def dtypes(self):
        return DTYPES3 if self.fp32_too else DTYPES16

    def plan_for(self, dtype):
        return dict(route="fp32", bm=128, bn=128, ksplit=1, form=0) if dtype == torch.float32 else self.plan

    def sample_rows(self, count):
        """at most `count` output rows, the first and last 64 among them (the CPU checks evaluate the references on these rows only)"""
        if self.m <= count:
            return torch.arange(self.m)
        mid = torch.arange(64, self.m - 64, max(1, (self.m - 128) // (count - 128)))
        return torch.cat([torch.arange(64), mid, torch.arange(self.m - 64, self.m)])


RING, TWO = "ring", "two-slot"


def _lin(name, plan, m, n, k, entry="gemm", **kw):
    return Case(name, "lin", plan, entry, m=m, n=n, k1=k, **kw)


def _conv(name, plan, b, h, w, cin, cout, entry="conv", **kw):
    return Case(name, "conv", plan, entry, n=cout, k1=cin, images=b, h=h, w=w, **kw)


_R = (RING, 256, 160, 1, 0)
_D0, _D1, _D2, _D3 = ("dualn", 256, 320, 1, 0), ("dualn", 256, 320, 1, 1), ("dualn", 256, 320, 1, 2), ("dualn", 256, 256, 1, 3)
CASES = [
    # ---- two-slot kernels (the first seven also run the fp32 twin, except the LayerNorm consumer, which launch_igemm_f32 refuses)
    _lin("ts64-ragged", (TWO, 64, 64, 1, 0), 100, 132, 128, res=True, fp32_too=True),
    _lin("ts64-splitk-time", (TWO, 64, 64, 5, 0), 72, 320, 1280, entry="conv", images=3, time=True, res=True, fp32_too=True),
    _lin("ts64-splitk-ln", (TWO, 64, 64, 5, 0), 72, 320, 1280, entry="gemm_ln", ln=True),
    _lin("ts64-f32out", (TWO, 64, 64, 1, 0), 3, 640, 128, entry="gemm_f32out", f32out=True, fp32_too=True),
    _lin("ts160", (TWO, 128, 160, 1, 0), 8232, 320, 128, fp32_too=True),
    _conv("ts160-deepk", (TWO, 128, 160, 8, 0), 4, 16, 16, 512, 1280, fp32_too=True),
    _lin("ts128-ragged", (TWO, 128, 128, 1, 0), 8168, 388, 128, res=True, fp32_too=True),
    _lin("ts128-geglu", (TWO, 128, 128, 1, 0), 136, 256, 128, geglu=True),
    _lin("ts128-geglu-ln", (TWO, 128, 128, 1, 0), 136, 256, 128, entry="gemm_ln", geglu=True, ln=True),
    _lin("ts64-per-image", (TWO, 64, 64, 1, 0), 384, 320, 128, entry="per_image", images=3, per_image=True),
    # ---- the 256 x 160 ring at its threshold of 144 tiles
    _lin("ring-k64-ragged", _R, 18376, 320, 64, res=True),
    _lin("ring-bare", _R, 4608, 1280, 192, bias=False),
    _lin("ring-lnprod", _R, 4608, 1280, 192, entry="gemm_ln", res=True, lnprod=True),
    _lin("ring-gnprod", _R, 4608, 1280, 192, entry="gemm_gn", images=18, res=True, gnprod=True),
    _lin("ring-ln", _R, 4608, 1280, 192, entry="gemm_ln", ln=True),
    _lin("ring-hm256", _R, 6144, 960, 320, entry="gemm_hm", ln=True, hm=256),
    _lin("ring-hm512", _R, 6144, 960, 320, entry="gemm_hm", ln=True, hm=512),
    _lin("ring-two-sources", _R, 4608, 1280, 64, entry="conv", k2=128, images=18, time=True),
    _lin("ring-per-image", _R, 4608, 1280, 128, entry="per_image", images=18, per_image=True, res=True),
    _conv("ring-stride2", _R, 18, 32, 32, 64, 1280, stride=2, time=True, res=True),
    _conv("ring-stride2-pad0", _R, 18, 32, 32, 64, 1280, entry="conv_ex", stride=2, pad0=1, res=True),
    _conv("ups9", ("ring-ups9", 256, 160, 1, 0), 18, 8, 8, 64, 1280, ups=1, time=True),
    _conv("ups4-image-major", ("ring-ups4", 256, 160, 1, 0), 5, 16, 16, 64, 1280, ups=2),
    _conv("ups4-phase-major-8", ("ring-ups4", 256, 160, 1, 0), 20, 8, 8, 64, 1280, ups=2),
    _conv("ups4-phase-major-24", ("ring-ups4", 256, 160, 1, 0), 4, 24, 24, 64, 1280, ups=2),
    _conv("patch-strided-time", ("ring-patch", 256, 160, 1, 0), 18, 16, 16, 64, 1280, time=True, time_strided=True, res=True),
    _conv("patch-gnprod", ("ring-patch", 256, 160, 1, 0), 18, 16, 16, 64, 1280, entry="conv_gn", time=True, res=True, gnprod=True),
    _conv("patch-16x32", ("ring-patch", 256, 160, 1, 0), 9, 16, 32, 64, 1280),
    _lin("ring-geglu", ("ring-geglu", 256, 128, 1, 0), 3328, 2560, 320, geglu=True),
    _lin("ring-geglu-ln", ("ring-geglu", 256, 128, 1, 0), 3328, 2560, 320, entry="gemm_ln", geglu=True, ln=True),
    # ---- the ping-pong kernels
    _conv("ppconv-256", ("ppconv", 256, 160, 1, 0), 25, 16, 16, 64, 1280),
    _conv("ppconv-dualm-gnprod", ("ppconv", 512, 160, 1, 1), 13, 32, 32, 64, 1280, entry="conv_gn", time=True, res=True, gnprod=True),
    _conv("ppconv-dualm-bare", ("ppconv", 512, 160, 1, 1), 13, 32, 32, 64, 1280, bias=False),
    _lin("dualn0-bias", _D0, 13312, 1280, 128),
    _lin("dualn0-res", _D0, 13312, 1280, 128, res=True),
    _lin("dualn0-lnprod", _D0, 13312, 1280, 128, entry="gemm_ln", res=True, lnprod=True),
    _lin("dualn0-gnprod", _D0, 13312, 1280, 128, entry="gemm_gn", images=52, res=True, gnprod=True),
    _lin("dualn0-two-sources", _D0, 13312, 1280, 128, entry="conv", k2=64, images=52),        # (c1 = 128: the dual-N kernel takes no first source below two K tiles)
    _lin("dualn0-two-rounds", _D0, 26368, 1280, 128),
    _lin("dualn1-ln", _D1, 13312, 1280, 128, entry="gemm_ln", ln=True),
    _lin("dualn2-hm40", _D2, 17664, 960, 128, entry="gemm_hm", ln=True, hm=256),
    _lin("dualn2-hm80", _D2, 8960, 1920, 128, entry="gemm_hm", ln=True, hm=256),
    _lin("dualn3-geglu-ln", _D3, 5376, 2560, 128, entry="gemm_ln", geglu=True, ln=True),
    # ---- the fp32 twin on the convs with a stride and an upsample, at 2 images (16-bit: 64 x 64 two-slot tiles)
    _conv("f32-stride2", (TWO, 64, 64, 1, 0), 2, 32, 32, 64, 1280, stride=2, time=True, res=True, fp32_too=True),
    _conv("f32-stride2-pad0", (TWO, 64, 64, 1, 0), 2, 32, 32, 64, 1280, entry="conv_ex", stride=2, pad0=1, res=True, fp32_too=True),
    _conv("f32-ups9", (TWO, 64, 64, 1, 0), 2, 8, 8, 64, 1280, ups=1, time=True, fp32_too=True),
]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)
PARAMS = [(c.name, dt, fam) for c in CASES for dt in c.dtypes() for fam in FAMILIES if not (c.geglu and fam == "exact")]


def param_id(p):
    return f"{p[0]}-{NAME[p[1]]}-{p[2]}"


# ---------------------------------------------------------------------------------------------------------------- the dispatch rule, restated
def route_rule(case, dtype):
    """igemm_route + launch_two_slot + the ping-pong launchers' tile choice at the default thresholds (ring 144 tiles, ppconv 192, dual-N 192 with a last
    round 80 % full, deep K 64 tiles / 64 K tiles, GEGLU ring K >= 320 and 256 tiles) -> the plan; None where launch_igemm refuses.  A premise check of the
    case list, as norm_ref.gn_geometry is of the norm cases: the GPU test asserts what the library itself reports"""
    c = case
    if dtype == torch.float32:
        return None if (c.ln or c.lnprod or c.gnprod or c.per_image or c.ups == 2) else dict(route="fp32", bm=128, bn=128, ksplit=1, form=0)
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    m, n, k = c.m, c.n, c.k1 + c.k2
    rpb = c.rows_per_image if (c.kind == "conv" or c.entry in ("conv", "gemm_gn", "per_image")) else m
    ring_fills = cdiv(m, 256) * cdiv(n, 160) >= 144
    ln_ring_ok = not c.ln or rpb % 64 == 0
    stat = c.lnprod or c.gnprod
    full80 = lambda tiles: tiles * 5 >= cdiv(tiles, 256) * 256 * 4  # noqa: E731
    plan = lambda route, bm, bn, ks=1, form=0: dict(route=route, bm=bm, bn=bn, ksplit=ks, form=form)  # noqa: E731
    if (c.taps == 9 and c.stride == 1 and not c.ups and not c.k2 and not c.pad0 and c.h % 16 == 0 and c.w % 16 == 0 and n % 160 == 0 and c.k1 % 64 == 0
            and not c.lnprod and (m // 256) * (n // 160) >= 192):
        dual_m = (m // 256) % 2 == 0 and full80((m // 512) * (n // 160))
        return plan("ppconv", 512 if dual_m else 256, 160, 1, int(dual_m))
    if c.taps == 1 and not c.time and not c.f32out and not c.per_image and m % 256 == 0 and c.k1 % 64 == 0 and c.k1 >= 128:
        ok = not (c.k2 and (c.geglu or c.ln or c.res or stat or c.k2 % 64)) and not (stat and rpb % 64)
        kind = -1
        if c.geglu:
            kind = 3 if (c.ln and not c.res and not stat and n % 256 == 0) else -1
        elif c.ln:
            kind = (2 if c.hm else 1) if (not c.res and not stat and n % 320 == 0) else -1
        elif n % 320 == 0:
            kind = 0
        tiles = (m // 256) * (n // (256 if kind == 3 else 320))
        if ok and kind >= 0 and tiles >= 192 and full80(tiles):
            return plan("dualn", 256, 256 if kind == 3 else 320, 1, kind)
    if c.ups == 2:
        hw = c.h * c.w
        ok = n % 160 == 0 and not (c.k2 or c.res or c.time or c.ln or c.pad0) and (hw % 256 == 0 or ((m >> 2) % 256 == 0 and hw % 64 == 0)) and ring_fills
        return plan("ring-ups4", 256, 160) if ok else None
    if c.hm and not (n % 160 == 0 and c.hm % 256 == 0 and m % c.hm == 0 and ln_ring_ok and ring_fills):
        return None
    if not c.geglu and c.ups == 1 and n % 160 == 0 and ring_fills:
        return plan("ring-ups9", 256, 160)
    if (not c.geglu and c.taps == 9 and c.stride == 1 and not c.ups and not c.k2 and not c.pad0 and c.h % 16 == 0 and c.w % 16 == 0 and n % 160 == 0
            and not c.ln and not c.f32out and not c.per_image and not c.lnprod and ring_fills):
        return plan("ring-patch", 256, 160)
    if not c.geglu and not c.ups and n % 160 == 0 and ring_fills and ln_ring_ok:
        return plan("ring", 256, 160)
    if c.geglu and ln_ring_ok and c.k1 >= 320 and cdiv(m, 256) * cdiv(n, 128) >= 256:
        return plan("ring-geglu", 256, 128)
    nk = c.taps * k // 64
    deep_k = not c.geglu and n % 160 == 0 and nk >= 64 and not c.f32out and cdiv(m, 128) * cdiv(n, 160) >= 64
    big = c.geglu or (cdiv(m, 128) * cdiv(n, 128) >= 192 and n > 64) or deep_k
    bm, bn = (128, 160) if (big and not c.geglu and n % 160 == 0) else (128, 128) if big else (64, 64)
    slots, tiles, ks = (1024 if bm == 64 else 512), cdiv(m, bm) * cdiv(n, bn), 1
    if not c.geglu and not c.f32out and tiles * 2 <= slots and nk >= 16:
        for d in range(2, 33):
            if nk % d == 0 and nk // d >= 4 and tiles * d <= slots and m * n * d * 4 <= 64 << 20:
                ks = d
    return plan("two-slot", bm, bn, ks)


def stat_report(case):
    """what the launch reports through stat_P: LayerNorm partials per row (80-column chunks on the ring and the dual-N kernel) / rows per GroupNorm partial"""
    return case.n // 80 if case.lnprod else 64 if case.gnprod else 0


# ---------------------------------------------------------------------------------------------------------------- operands
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _mix(x):
    """a 32-bit integer hash (two multiply-xorshift rounds) of an int64 tensor"""
    x = x & 0xFFFFFFFF
    for _ in range(2):
        x = ((x ^ (x >> 16)) * 0x45D9F3B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def hash_ternary(shape, salt, density):
    """values in {-1, 0, 1}, non-zero with probability `density`, from a hash of the flat index"""
    h = _mix(torch.arange(math.prod(shape), dtype=torch.int64) + salt * 0x9E3779B1)
    sign = 1 - 2 * ((h >> 20) & 1)
    return (sign * ((h & 1023) < int(density * 1024))).reshape(shape).float()


def hash_int(shape, salt, lim):
    """integers in [-lim, lim] from the same hash"""
    h = _mix(torch.arange(math.prod(shape), dtype=torch.int64) + salt * 0x9E3779B1)
    return ((h >> 3) % (2 * lim + 1) - lim).reshape(shape).float()


def exact_w_density(k_total):
    return min(2.0 / 3.0, 96.0 / k_total)


@functools.lru_cache(maxsize=3)
def _shape_operands(key, taps, dtype, family):
    """every operand any epilogue variant of a shape reads, on the CPU in the kernel's types (cases that share a shape share these: the cache is keyed by
    Case.shape_key): a [rows_in][k1 + k2], w [n][taps][k1 + k2] ([images n][k] per image; ups 2: the packed phase weights, and w32 [n][cin][3][3], the fp32
    originals), bias / c [n] ([images][n] per image), time [images][n], res [m][n], stat [m][2], s [n]"""
    kind, m, n, k1, k2, images, h, w, stride, ups, pad0, per_image = key
    rows_in = images * h * w if kind == "conv" else m
    kt = taps * (k1 + k2)
    wshape = (images * n, k1 + k2) if per_image else (n, 9, k1) if ups == 2 else (n, taps, k1 + k2)
    o = types.SimpleNamespace()
    if family == "random":
        g = _gen(key, "random")
        o.a = torch.randn(rows_in, k1 + k2, generator=g)
        o.w = torch.randn(wshape, generator=g) * (9 * k1 if ups == 2 else kt) ** -0.5
        o.bias = torch.randn(images if per_image else 1, n, generator=g) + 0.5
        o.time = torch.randn(images, n, generator=g) + 0.75 * torch.arange(images).float()[:, None]
        o.res = 2.0 * torch.randn(m, n, generator=g)
        i = torch.arange(m)
        mean = (1.5 + 0.5 * (i % 4)) * (1 - 2 * ((i // 2) % 2)).float()
        rstd = torch.tensor([0.5, 2.0, 1.0])[i % 3] * (1 + 0.05 * torch.randn(m, generator=g))
        o.stat = torch.stack([mean, rstd], dim=1).float()
        o.s = torch.randn(n, generator=g)
    else:
        o.a = hash_ternary((rows_in, k1 + k2), 1, 2.0 / 3.0)
        o.w = hash_ternary(wshape, 2, exact_w_density(kt if ups != 2 else 9 * k1))
        # the scalar operands are linear congruences: a step of one row, column or image (and of a 16-, 64-, 80-, 160- or 256-wide tile) always changes them
        i, j = torch.arange(m)[:, None], torch.arange(n)[None, :]
        img = torch.arange(images)[:, None]
        o.bias = (((5 * j + 3 * img) % 17) - 8).float()[: images if per_image else 1]
        o.time = (((7 * j + 5 * img) % 17) - 8).float()
        o.res = (((3 * i + 7 * j) % 33) - 16).float()
        i = i[:, 0]
        mean = (1 + 2 * (hash_int((m,), 6, 1) > 0) + i % 2) * (1 - 2 * ((i // 2) % 2))          # 1 or 3 on even rows, 2 or 4 on odd rows, signs in pairs
        o.stat = torch.stack([mean.float(), torch.tensor([0.5, 2.0, 1.0])[i % 3]], dim=1)
        o.s = (((3 * j[0]) % 7) - 3).float()
    o.a, o.res = o.a.to(dtype), o.res.to(dtype)
    if ups == 2:
        o.w32 = o.w.reshape(n, 3, 3, k1).permute(0, 3, 1, 2).contiguous()            # [n][cin][3][3] fp32, what etainv_op_pack_ups4 reads
        o.w = pack_ups4_ref(o.w32, dtype)
    else:
        o.w = o.w.to(dtype)
    if not per_image:
        o.bias = o.bias[0]
    return o


# ---------------------------------------------------------------------------------------------------------------- references
def accumulate(case, a, a2, w, dt, rows=None, want_abs=True, fault=None):
    """acc = A W^T (and sum |a||w|) for output rows `rows` (all by default), computed in `dt` from operands on any device.  a / a2: the activation rows as
    the kernel reads them ([rows_in][k1], [rows_in][k2]); w as in shape_operands.  fault: "ktile" drops the second K tile of 64; "tap" shifts a border tap"""
    c = case
    dev = a.device
    rows = torch.arange(c.m, device=dev) if rows is None else rows.to(dev)
    x = a.to(dt) if a2 is None else torch.cat([a.to(dt), a2.to(dt)], dim=1)
    k = x.shape[1]

    def mm(av, wv):
        if fault == "ktile":
            av = av.clone()
            av[:, 64:128] = 0
        return (av @ wv.t(), av.abs() @ wv.abs().t() if want_abs else None)

    if c.kind == "lin":
        if c.per_image:
            img = rows // c.rows_per_image
            wv = w.to(dt).reshape(c.images, c.n, k)
            acc = torch.empty(len(rows), c.n, dtype=dt, device=dev)
            ab = torch.empty_like(acc) if want_abs else None
            for i in range(c.images):
                sel = img == i
                if bool(sel.any()):
                    r = mm(x[rows[sel]], wv[i])
                    acc[sel] = r[0]
                    if want_abs:
                        ab[sel] = r[1]
            return acc, ab
        return mm(x[rows], w.to(dt).reshape(c.n, k))
    xp = torch.cat([x.reshape(c.images, c.h * c.w, k), torch.zeros(c.images, 1, k, dtype=dt, device=dev)], dim=1)
    img, pix = rows // c.rows_per_image, rows % c.rows_per_image
    shift = 0 if fault == "tap" else None
    if c.ups != 2:
        idx = tap_index(c.h, c.w, c.ho, c.wo, c.stride, 0 if c.pad0 else 1, c.ups, TAPS9, shift).to(dev)
        return mm(xp[img[:, None], idx[pix]].reshape(len(rows), 9 * k), w.to(dt).reshape(c.n, 9 * k))
    acc = torch.empty(len(rows), c.n, dtype=dt, device=dev)
    ab = torch.empty_like(acc) if want_abs else None
    oy, ox = pix // c.wo, pix % c.wo
    for ph in range(4):
        py, px = ph >> 1, ph & 1
        sel = (oy % 2 == py) & (ox % 2 == px)
        if not bool(sel.any()):
            continue
        idx = tap_index(c.h, c.w, c.h, c.w, 1, 1, 0, phase_taps(py, px), shift).to(dev)
        src = (oy[sel] // 2) * c.w + ox[sel] // 2
        r = mm(xp[img[sel][:, None], idx[src]].reshape(int(sel.sum()), 4 * k), w[ph].to(dt).reshape(c.n, 4 * k))
        acc[sel] = r[0]
        if want_abs:
            ab[sel] = r[1]
    return acc, ab


def _epilogue_terms(case, o, rows, dt, fault=None):
    """(bias or c, time, residual, mean, rstd, s), each broadcastable to [rows][n] in `dt`, None where the case has none; o: the operands on the device of
    `rows`.  Faults: bias of column n + 1, residual of row m + 1, stat of row m + 1"""
    c = case
    img = rows // c.rows_per_image
    roll = lambda t, d: torch.roll(t, -1, dims=d)  # noqa: E731
    bias = None
    if c.bias or c.ln:
        b = o.bias.to(dt)
        if fault == "bias":
            b = roll(b, -1)
        bias = b[img] if c.per_image else b[None, :]
    time = o.time.to(dt)[img] if c.time else None
    res = None
    if c.res:
        r = o.res.to(dt)[:, : c.n_out]
        res = (roll(r, 0) if fault == "res" else r)[rows]
    mean = rstd = s = None
    if c.ln:
        st = o.stat.to(dt)
        st = (roll(st, 0) if fault == "stat" else st)[rows]
        mean, rstd, s = st[:, 0:1], st[:, 1:2], o.s.to(dt)[None, :]
    return bias, time, res, mean, rstd, s


def reference(case, o, dtype, ksplit, rows=None, prod=None):
    """-> (ref, bound, e) float64 [rows][n_out] for operands o on any device; dtype: the operand type (the stored type, fp32 with f32out); prod: what
    accumulate(...) gave for these operands and rows, where the caller shares it among the epilogue variants of a shape"""
    c = case
    acc, ab = prod if prod is not None else accumulate(c, o.a1, o.a2, o.w, torch.float64, rows)
    rows = torch.arange(c.m, device=acc.device) if rows is None else rows.to(acc.device)
    bias, time, res, mean, rstd, s = _epilogue_terms(c, o, rows, torch.float64)
    gl = gamma_l(c.k_total + ksplit + 4)
    if c.ln:
        h = rstd * (acc - mean * s) + bias
        e = gl * (rstd.abs() * (ab + (mean * s).abs()) + bias.abs())
    else:
        h, mag = acc, ab
        for t in (bias, time, res):
            if t is not None:
                h, mag = h + t, mag + t.abs()
        e = gl * mag
    if c.geglu:
        (a, g), (ea, eg) = geglu_split(h), geglu_split(e)
        gel = gelu64(g)
        e_gelu = GELU_LIP * eg + 0.5 * g.abs() * ERF_ERR + 2 * U32 * gel.abs()
        h = a * gel
        e = a.abs() * e_gelu + gel.abs() * ea + ea * e_gelu + U32 * h.abs()
    out_t = torch.float32 if c.f32out else dtype
    return h, U_RND[out_t] * (h.abs() + e) + e + ABS_FLOOR[out_t], e


def emulate(case, o, rows=None, fault=None):
    """fp32 matmul of the same operands, the epilogue in fp32 in the kernel's order ((acc - mean s) rstd + c; acc + bias + time row + residual; a gelu_pair(g)),
    BEFORE the rounding to the stored type"""
    c = case
    acc, _ = accumulate(c, o.a1, o.a2, o.w, torch.float32, rows, want_abs=False, fault=fault if fault in ("ktile", "tap") else None)
    rows = torch.arange(c.m, device=acc.device) if rows is None else rows.to(acc.device)
    bias, time, res, mean, rstd, s = _epilogue_terms(c, o, rows, torch.float32, fault)
    v = (acc - mean * s) * rstd if c.ln else acc
    for t in (bias, time, res):
        if t is not None:
            v = v + t
    if c.geglu:
        a, g = geglu_split(v)
        v = a * gelu_pair_emu(g)
    return v


def case_operands(case, dtype, family, device="cpu"):
    """the operands of one case on `device`: a1 / a2 split off the shared activation rows, the rest shared by reference"""
    s = _shape_operands(case.shape_key, case.taps, dtype, family)
    o = types.SimpleNamespace(**{k: (v.to(device) if torch.is_tensor(v) else v) for k, v in vars(s).items()})
    o.a1 = o.a[:, : case.k1].contiguous()
    o.a2 = o.a[:, case.k1:].contiguous() if case.k2 else None
    return o


# ---------------------------------------------------------------------------------------------------------------- producer partials
LN_CHUNK, LN_LANE = 80, 20          # an 80-column wave tile per partial; each of four lanes holds 20 of its values
GN_ROWS = 64


def ln_partials64(stored):
    """stored [m][n] (the kernel's own output) -> float64 (mean, M2) [m][n / 80][2]"""
    ch = stored.double().reshape(stored.shape[0], -1, LN_CHUNK)
    mean = ch.mean(-1)
    return torch.stack([mean, ((ch - mean[..., None]) ** 2).sum(-1)], dim=-1)


def ln_partial_err(stored):
    """(dmean, dM2) [m][n / 80] of emit_row_stat (csrc/igemm.hip; csrc/ppgemm.hip does the same): per lane the fp32 sum of its 20 values (19 additions), times
    fl(1 / 20) (2 roundings), M2_lane = sum fl(fl(x - mu)^2) (3 roundings a term, 20 additions); two Chan merges of equal counts, each d = fl(mb - ma),
    mean = fl(ma + d / 2), M2 = fl(fl(qa + qb) + fl(fl(d d) fl(n / 2))).  Which columns a lane holds does not enter: with A = max |x| and R = max - min of the
    chunk, dmu_lane <= 21 u A, a deviation is at most R, and a sum of squares about a pivot off by dmu gains count dmu^2 (the first-order term vanishes).
    In the manner of norm_ref.ln_finalize_err"""
    ch = stored.double().reshape(stored.shape[0], -1, LN_CHUNK)
    a, r = ch.abs().amax(-1), ch.amax(-1) - ch.amin(-1)
    mean = ch.mean(-1)
    m2 = ((ch - mean[..., None]) ** 2).sum(-1)
    dm = 21 * U32 * a
    # lane level: every term carries 3 roundings and the chain 20 more; the four lanes' M2 sum to at most M2
    dq = gamma_l(23) * (m2 + LN_CHUNK * dm ** 2) + LN_CHUNK * dm ** 2
    for n_side in (20.0, 40.0):
        dd = 2 * dm + U32 * (r + 2 * dm)                                         # error of d' = fl(mb' - ma') against mb - ma
        t_up = (r + dd) ** 2 * n_side / 2
        dq = dq + (2 * r * dd + dd * dd) * n_side / 2 * (LN_CHUNK / (2 * n_side)) + (3 * U32 * t_up + 2 * U32 * (m2 + dq + t_up)) * (LN_CHUNK / (2 * n_side))
        dm = dm + 0.5 * U32 * (r + 2 * dm) + U32 * (a + dm)                      # mean' = (ma' + mb') / 2 + the rounding of d' / 2 + the addition's
    return dm, dq


def patch_rows(images, h, w, device="cpu"):
    """the VIRTUAL row order of the patch kernels (ppconv, ring-patch), whose M tile is a 16 x 16 pixel patch: images, then an image's patches row by row,
    then the patch's 16 rows of 16 pixels -> the NHWC row of every virtual row.  Their GroupNorm partials are over 64 consecutive virtual rows (4 patch rows)"""
    b, py, px, y, x = torch.meshgrid(torch.arange(images, device=device), torch.arange(h // 16, device=device), torch.arange(w // 16, device=device),
                                     torch.arange(16, device=device), torch.arange(16, device=device), indexing="ij")
    return ((b * h + py * 16 + y) * w + px * 16 + x).flatten()


def gn_partials64(stored):
    """stored [m][n] -> float64 [m / 64][2][n]: per channel the sum and the sum of squares over each block of 64 stored rows"""
    blk = stored.double().reshape(-1, GN_ROWS, stored.shape[1])
    return torch.stack([blk.sum(1), (blk * blk).sum(1)], dim=1)


def gn_partial_err(stored):
    """the bound of a chain of 64 fp32 additions (65 with the product x x), any order: [m / 64][2][n]"""
    blk = stored.double().reshape(-1, GN_ROWS, stored.shape[1])
    return torch.stack([gamma_l(GN_ROWS) * blk.abs().sum(1), gamma_l(GN_ROWS + 1) * (blk * blk).sum(1)], dim=1)
