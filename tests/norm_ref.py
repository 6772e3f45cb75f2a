"""Plain-PyTorch references for the norm kernels (csrc/norm.hip, their fp32 twins in csrc/f32path.hip) and the statistics hand-over between GEMM epilogues and
norms -- no GPU needed, no import of the library.  Everything here is device-agnostic torch: tests/test_norm_ref.py runs it on the CPU, tests/test_norm_gpu.py on
the device (float64 there too), on the SAME inputs, which the case lists at the end of this module define.

  references   float64 GroupNorm(+SiLU) over NHWC cat[x1, x2] for any `groups`, LayerNorm, row statistics, Chan's merge of (mean, M2) partials of equal count,
               GroupNorm statistics (and the scale / shift planes [b][2][C]) from per-channel (sum, sum of squares) row-block partials.  All on inputs already
               rounded to the io type, with eps rounded to fp32 as the kernels receive it.
  partials     gn_partials / ln_partials: fp32 roundings of float64 block sums / chunk (mean, M2).  The references work from these same fp32 values in float64,
               so that only the kernel's own arithmetic is measured.
  geometry     gn_geometry restates launch_groupnorm: chunks, chunks_apply, pixels per chunk, the fp32 addition chain, the stats / apply instantiation.
  emulation    the best the kernel's expression can do: y = fma(x, sc, sh) in fp32 with sc = rstd gamma, sh = fma(-mean, sc, beta) from float64 statistics rounded
               to fp32 (a product and the sum behind it contracted, as the compiler may), SiLU through exp2 in fp32, ONE rounding to the io type; for the 16-bit
               GroupNorm also the fp32 E[x^2] - mean^2 summation in the kernel's order.
  bounds       per element, by counting roundings (u = 2^-24, the worst relative error of one fp32 operation):
                 |out - ref| <= U_RND (|ref| + e) + e + floor,     e = SiLU(e_y),   e_y = N_EXPR u A + dmean rstd |gamma| + |n gamma| drstd
               with n = (x - mean) rstd, A = (|x| + |mean|) rstd |gamma| + |beta| (what the fp32 terms of the expression round against), dmean / drstd the
               absolute / relative error of the statistics (below), U_RND one rounding to the io type, floor half an fp16 subnormal step.

Counting.  N_EXPR = 6: the 16-bit kernels compute sc = fl(rstd32 gamma) (rstd32 and the product: 2 u on every term that holds sc), sh = fl(beta - fl(mean32 sc))
(mean32, the product and the difference), y = fl(fl(x sc) + sh): |x sc| carries 2 + 1 + 1 roundings, |mean sc| 1 + 2 + 1 + 1 + 1 = 6, |beta| 2.  The fp32 twins
and LayerNorm compute fl(fl(fl(fl(x - mean32) rstd32) gamma) + beta): at most 5 on any term.
Statistics of the 16-bit GroupNorm: per-channel fp32 running sums of x and fl(x x) over a wave's pixels of a chunk, then fp32 sums over the 4 waves and a group's
channels in LDS; everything behind that is double.  The longest addition chain is L = geometry.chain, so |sum' - sum| <= g_L sum|x|, g_L = L u / (1 - L u), and
  dmean = g_L E|x|,   dvar = g_L E[x^2] + 2 |mean| dmean + dmean^2,   drstd = max((v / max(v - dvar, eps))^1/2 - 1, 1 - (v / (v + dvar))^1/2),  v = var + eps
(the kernels clamp the variance at zero) -- first order L u (mean^2 + var) / (var + eps) times at most 3/2: the condition number of var = E[x^2] - mean^2.  `centred = True` evaluates the same formulas on
the group with its mean removed: the bound of a kernel that is as good on an offset group as on a centred one.
The fp32 GroupNorm and the finalize of the producer partials sum in double: dmean = STAT_CONV u |mean|, drstd = STAT_CONV u (one conversion to fp32 each, one
spare).  LayerNorm and row_stats are two-pass: L_ROW = 24 + 6 (three vectors of 8 per lane, 6 butterfly steps; the fp32 twin: 20 + 6), dmean = (L_ROW + 1) u E|x|,
var + eps carries L_ROW + 5 roundings plus dmean^2 (the first-order term of a wrong pivot vanishes), rsqrt 2 u.
SiLU: |silu'| <= SILU_LIP = 1.1 (its maximum is 1.0998 at y = 2.4); the fp32 evaluation y / (1 + exp2(-y log2 e)) against float64 measured
SILU_MEASURED = 2.04 in units of u (1 + |y|) |silu(y)| over y in [-30, 30] (measure_silu_error; the (1 + |y|) is the rounding of the exponent's argument), and
the bound takes K_SILU = 2 x that figure.
Short chains.  A count of one to three roundings is attained on some of a thousand rows, so no emulation stays inside half of it.  The bounds of such values --
the planes of gn_finalize_kernel, var + eps and the rsqrt at the end of ln_finalize_kernel -- are SHORT = 2 times their count, as STAT_CONV is twice the one
conversion (the convention of R_ULP in tests/test_aux_kernels_gpu.py: one ulp, twice the worst rounding).
The emulation and the factor one half.  A value rounded once to the io type sits, over a few thousand elements, AT U_RND |ref|: no emulation that rounds can use
half of a bound whose first term is that one rounding.  So the emulations return fp32, before the output rounding, and the condition of tests/test_norm_ref.py is
|emulation - ref| <= e / 2 on the part e of the bound in front of the rounding (every bound function returns (ref, bound, e)); rounding then adds at most
U_RND (|ref| + e / 2), and the rounded emulation stays inside `bound`, which the same test asserts too."""
import functools
import types

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
U_RND = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 0.0}          # = U_RND of tests/test_aux_kernels_gpu.py
ABS_FLOOR = {torch.float16: 2.0 ** -25, torch.bfloat16: 0.0, torch.float32: 0.0}          # half an fp16 subnormal step
N_EXPR = 6
STAT_CONV = 2
SHORT = 2
L_ROW = 30
SILU_LIP = 1.1
SILU_MEASURED = 2.04
K_SILU = 2 * SILU_MEASURED
LOG2E = 1.4426950408889634
GN_MAX_CHUNKS = 64
DTYPES16 = [torch.float16, torch.bfloat16]
DTYPES3 = [torch.float16, torch.bfloat16, torch.float32]
NAME = {torch.float16: "fp16", torch.bfloat16: "bf16", torch.float32: "fp32"}


def f32(v):
    """a Python float rounded to fp32 (eps as the kernels receive it)"""
    return float(torch.tensor(v, dtype=torch.float32))


def per_channel(stat, cpg):
    """[b][groups] -> [b][1][C]"""
    return stat.repeat_interleave(cpg, dim=1)[:, None, :]


# ---------------------------------------------------------------------------------------------------------------- float64 references
def ref_gn_stats(x, groups, eps):
    """x [b][hw][C] -> (mean, var, rstd), each [b][groups], float64, two-pass"""
    b, hw, c = x.shape
    g = x.double().reshape(b, hw, groups, c // groups)
    mean = g.mean((1, 3))
    var = ((g - mean[:, None, :, None]) ** 2).mean((1, 3))
    return mean, var, (var + f32(eps)).rsqrt()


def ref_groupnorm(x, gamma, beta, groups, eps, silu, stats=None):
    """x [b][hw][C] (the concatenation of the sources) -> float64 [b][hw][C]; `stats` = (mean, rstd) [b][groups] to normalise with given statistics"""
    cpg = x.shape[-1] // groups
    if stats is None:
        mean, _, rstd = ref_gn_stats(x, groups, eps)
    else:
        mean, rstd = stats
    y = (x.double() - per_channel(mean.double(), cpg)) * per_channel(rstd.double(), cpg) * gamma.double() + beta.double()
    return F.silu(y) if silu else y


def ref_row_stats(x, eps):
    """x [rows][c] -> (mean, var, rstd) [rows], float64"""
    x = x.double()
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    return mean, var, (var + f32(eps)).rsqrt()


def ref_layernorm(x, gamma, beta, eps):
    mean, _, rstd = ref_row_stats(x, eps)
    return (x.double() - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double()


def chan_merge(part, cw, eps):
    """part [rows][P][2] = (mean, M2) of P chunks of cw columns each -> (mean, rstd) [rows] of the whole row, float64, Chan's update in index order"""
    part = part.double()
    n = 0.0
    mean = torch.zeros_like(part[:, 0, 0])
    m2 = torch.zeros_like(mean)
    for q in range(part.shape[1]):
        d = part[:, q, 0] - mean
        mean = mean + d * (cw / (n + cw))
        m2 = m2 + part[:, q, 1] + d * d * (n * cw / (n + cw))
        n += cw
    return mean, (m2 / n + f32(eps)).rsqrt()


def gn_from_partials(p1, wm1, p2, wm2, b, hw, groups, eps, gamma, beta):
    """p [b hw / wm][2][c] per-channel (sum, sum of squares) of row blocks of wm pixels -> (mean, rstd) [b][groups] and the scale / shift planes [b][2][C] that
    launch_groupnorm_pre writes behind them, float64"""
    sums = [p.double().reshape(b, hw // wm, 2, p.shape[-1]).sum(1) for p, wm in ((p1, wm1), (p2, wm2)) if p is not None]
    s = torch.cat(sums, dim=-1)                                                              # [b][2][C]
    c = s.shape[-1]
    cpg = c // groups
    count = float(hw * cpg)
    a, q = s[:, 0].reshape(b, groups, cpg).sum(-1), s[:, 1].reshape(b, groups, cpg).sum(-1)
    mean = a / count
    var = (q / count - mean * mean).clamp_min(0.0)
    rstd = (var + f32(eps)).rsqrt()
    sc = rstd.repeat_interleave(cpg, 1) * gamma.double()
    sh = beta.double() - mean.repeat_interleave(cpg, 1) * sc
    return mean, rstd, torch.stack([sc, sh], dim=1)


# ---------------------------------------------------------------------------------------------------------------- partial builders
def gn_partials(x, wm):
    """x [b][hw][c] (io type) -> fp32 [b hw / wm][2][c], the roundings of the float64 block sums"""
    b, hw, c = x.shape
    assert hw % wm == 0
    blk = x.double().reshape(b * hw // wm, wm, c)
    return torch.stack([blk.sum(1), (blk * blk).sum(1)], dim=1).float().contiguous()


def ln_partials(x, p):
    """x [rows][c] -> fp32 [rows][P][2], the roundings of the float64 (mean, M2) of P chunks of c / P columns"""
    rows, c = x.shape
    assert c % p == 0
    ch = x.double().reshape(rows, p, c // p)
    mean = ch.mean(-1)
    return torch.stack([mean, ((ch - mean[..., None]) ** 2).sum(-1)], dim=-1).float().contiguous()


# ---------------------------------------------------------------------------------------------------------------- launch geometry
def gn_geometry(b, hw, c1, c2=0, groups=32, apply_blocks=2048, noflat=False):
    """launch_groupnorm (16-bit) with the defaults of ETAINV_GN_APPLY_BLOCKS / ETAINV_GN_NOFLAT"""
    c = c1 + c2
    nvec = c // 8
    cpg = c // groups
    chunks = min(GN_MAX_CHUNKS, max(1, min(hw // 8, 1024 // max(1, b))))
    chunks_apply = max(1, min(hw // 4, max(chunks, apply_blocks // max(1, b))))
    per, per_apply = -(-hw // chunks), -(-hw // chunks_apply)
    chain_pixels = -(-min(per, hw) // 4)                        # wave 0 of a full chunk
    lds_adds = 4 * -(-cpg // 8) + 3 if groups <= 32 else 4 * cpg
    return types.SimpleNamespace(
        chunks=chunks, chunks_apply=chunks_apply, per=per, per_apply=per_apply, cpg=cpg,
        empty_stats=[k for k in range(chunks) if k * per >= hw], empty_apply=[k for k in range(chunks_apply) if k * per_apply >= hw],
        stats_vpl=min(5, (nvec + 63) // 64), apply_mode=0 if (not noflat and nvec in (40, 80)) else min(5, (nvec + 63) // 64),
        wide_groups=groups > 32, chain_pixels=chain_pixels, lds_adds=lds_adds,
        chain=chain_pixels + 1 + lds_adds)                      # + 1: the product x x of the sum of squares


# ---------------------------------------------------------------------------------------------------------------- emulation
def fma(a, b, c):
    """fp32 a b + c with one rounding, as the compiler contracts it (the product of two fp32 values is exact in float64; the second rounding of the float64
    sum moves the result by 2^-29 of an fp32 rounding at the most)"""
    return (a.double() * b.double() + c.double()).float()


def silu_emu(y, exact_exp=False):
    """fp32: y / (1 + exp2(-y log2 e)) as silu_f (__expf) evaluates it; exact_exp: expf, the fp32 twins"""
    y = y.float()
    e = torch.exp(-y) if exact_exp else torch.exp2(-y * f32(LOG2E))
    return y / (1.0 + e)


def measure_silu_error(lo=-30.0, hi=30.0, n=600001):
    """worst |silu_emu - silu64| / (u (1 + |y|) |silu64|) over fp32 y in [lo, hi]"""
    y = torch.linspace(lo, hi, n, dtype=torch.float64).float()
    y = y[y != 0]
    ref = F.silu(y.double())
    return float(((silu_emu(y).double() - ref).abs() / (U32 * (1 + y.double().abs()) * ref.abs())).max())


def emulate_gn_stats16(x, groups, eps, geo):
    """gn_stats_kernel + the reduction in front of gn_apply_kernel, in their order: fp32 per-channel running sums over pixels beg + w, beg + w + 4, ... of every
    (chunk, wave w), fp32 sums over waves and a group's channels (eight strided threads and a butterfly; one thread per group when groups > 32), double from
    there on.  x [b][hw][C] -> (mean, rstd) fp32 [b][groups]"""
    xf = x.float()
    b, hw, c = xf.shape
    cpg = c // groups
    k, w = torch.arange(geo.chunks, device=x.device), torch.arange(4, device=x.device)
    beg = k * geo.per
    end = (beg + geo.per).clamp(max=hw)
    s = torch.zeros(b, geo.chunks, 4, c, dtype=torch.float32, device=x.device)
    q = torch.zeros_like(s)
    for i in range(geo.chain_pixels):
        pix = beg[:, None] + w[None, :] + 4 * i
        ok = (pix < end[:, None])[None, :, :, None]
        t = torch.where(ok, xf[:, pix.clamp(max=hw - 1)], torch.zeros((), dtype=torch.float32, device=x.device))
        s = s + t
        q = q + t * t
    out = []
    for sm in (s, q):
        sm = sm.reshape(b, geo.chunks, 4, groups, cpg)
        if groups <= 32:
            part = []
            for sub in range(8):
                a = torch.zeros(b, geo.chunks, groups, dtype=torch.float32, device=x.device)
                for wv in range(4):
                    for ch in range(sub, cpg, 8):
                        a = a + sm[:, :, wv, :, ch]
                part.append(a)
            a = ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]))
        else:
            a = torch.zeros(b, geo.chunks, groups, dtype=torch.float32, device=x.device)
            for wv in range(4):
                for ch in range(cpg):
                    a = a + sm[:, :, wv, :, ch]
        out.append(a.double().sum(1))
    count = float(hw * cpg)
    mean = out[0] / count
    var = (out[1] / count - mean * mean).clamp_min(0.0)
    return mean.float(), (1.0 / (var + f32(eps)).sqrt()).float()


def emulate_scsh(mean32, rstd32, gamma, beta, cpg):
    """fp32 [b][C] each: sc = fl(rstd gamma), sh = fma(-mean, sc, beta)"""
    sc = rstd32.float().repeat_interleave(cpg, 1) * gamma.float()
    return sc, fma(-mean32.float().repeat_interleave(cpg, 1), sc, beta.float())


def emulate_affine(x, sc, sh, silu):
    """y = fma(x, sc, sh), SiLU; fp32, BEFORE the rounding to the io type"""
    y = fma(x.float(), sc[:, None, :], sh[:, None, :])
    return silu_emu(y) if silu else y


def emulate_groupnorm(x, gamma, beta, groups, eps, silu, dtype, geo=None, stats=None):
    """16-bit types: the statistics as the kernel sums them (geo given), or `stats` = (mean, rstd) float64 rounded to fp32, then x sc + sh.
    fp32: float64 statistics rounded to fp32, fma(fl(fl(x - mean) rstd), gamma, beta), expf.  Returns fp32, before the rounding to the io type"""
    cpg = x.shape[-1] // groups
    if stats is None:
        if dtype != torch.float32 and geo is not None:
            stats = emulate_gn_stats16(x, groups, eps, geo)
        else:
            mean, _, rstd = ref_gn_stats(x, groups, eps)
            stats = (mean, rstd)
    mean32, rstd32 = stats[0].float(), stats[1].float()
    if dtype == torch.float32:
        y = fma((x.float() - per_channel(mean32, cpg)) * per_channel(rstd32, cpg), gamma.float(), beta.float())
        return silu_emu(y, exact_exp=True) if silu else y
    return emulate_affine(x, *emulate_scsh(mean32, rstd32, gamma, beta, cpg), silu)


def wave_sum_emu(v):
    """v [rows][k][64] fp32: every lane adds its k values in order, then the xor butterfly 32, 16, ... 1 -> [rows]"""
    a = torch.zeros_like(v[:, 0])
    for i in range(v.shape[1]):
        a = a + v[:, i]
    lanes = torch.arange(64, device=v.device)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[:, lanes ^ o]
    return a[:, 0]


def _lanes(x, dtype):
    """the (value, lane) ownership of layernorm_kernel / row_stats_kernel (vectors of 8: lane l owns vectors l, l + 64, l + 128) and of layernorm_f32_kernel
    (lane l owns columns l, l + 64, ...): [rows][k][64], zero where a lane owns nothing"""
    rows, c = x.shape
    if dtype == torch.float32:
        return F.pad(x.float(), (0, 1280 - c)).reshape(rows, 20, 64)
    return F.pad(x.float(), (0, 1536 - c)).reshape(rows, 3, 64, 8).permute(0, 1, 3, 2).reshape(rows, 24, 64)


def emulate_row_stats(x, eps, dtype):
    """two-pass fp32 (mean, rstd) [rows] in the kernels' order"""
    c = x.shape[1]
    v = _lanes(x, dtype)
    own = _lanes(torch.ones_like(x, dtype=torch.float32), dtype) > 0
    mean = wave_sum_emu(v) / float(c)
    d = torch.where(own, v - mean[:, None, None], torch.zeros((), dtype=torch.float32, device=x.device))
    var = wave_sum_emu(d * d) / float(c) + f32(eps)
    return mean, (1.0 / var.sqrt() if dtype == torch.float32 else var.rsqrt())


def emulate_layernorm(x, gamma, beta, eps, dtype):
    mean, rstd = emulate_row_stats(x, eps, dtype)
    return fma((x.float() - mean[:, None]) * rstd[:, None], gamma.float(), beta.float())


def emulate_ln_finalize(part, cw, eps):
    """ln_finalize_kernel in fp32, operation by operation"""
    part = part.float()
    cw = float(cw)
    n = 0.0
    mean = torch.zeros_like(part[:, 0, 0])
    m2 = torch.zeros_like(mean)
    for q in range(part.shape[1]):
        nt = n + cw
        f = f32(cw / nt)
        d = part[:, q, 0] - mean
        mean = mean + d * f
        m2 = m2 + (part[:, q, 1] + d * d * n * f)
        n = nt
    return mean, (m2 / n + f32(eps)).rsqrt()


def emulate_gemm_ln(x, wp, s_vec, c_vec, mean32, rstd32):
    """the folded-LayerNorm consumer: fp32 accumulation of the 16-bit products, fl(rstd (acc - mean s[n]) + c[n]); before the output rounding"""
    acc = x.float() @ wp.float().t()
    return rstd32.float()[:, None] * (acc - mean32.float()[:, None] * s_vec.float()) + c_vec.float()


# ---------------------------------------------------------------------------------------------------------------- bounds
def gamma_l(length):
    return length * U32 / (1 - length * U32)


def rstd_err(dvar, v, eps):
    """relative error of (v' )^-1/2 against v^-1/2 for v = var + eps and |v' - v| <= dvar; the kernels clamp the variance at zero, so v' >= eps"""
    return torch.maximum((v / (v - dvar).clamp_min(f32(eps))).sqrt() - 1, 1 - (v / (v + dvar)).sqrt())


def gn_stats_err16(x, groups, eps, geo, centred=False):
    """(dmean, drstd) [b][groups] of the fp32 E[x^2] - mean^2 summation (module docstring); centred: of the same group with its mean removed"""
    b, hw, c = x.shape
    g = x.double().reshape(b, hw, groups, c // groups)
    mean = g.mean((1, 3))
    var = ((g - mean[:, None, :, None]) ** 2).mean((1, 3))
    if centred:
        g = g - mean[:, None, :, None]
        mean = torch.zeros_like(mean)
    gl = gamma_l(geo.chain)
    dmean = gl * g.abs().mean((1, 3))
    dvar = gl * (g * g).mean((1, 3)) + 2 * mean.abs() * dmean + dmean ** 2
    return dmean, rstd_err(dvar, var + f32(eps), eps)


def stats_err_double(mean):
    """(dmean, drstd) of statistics summed in double and converted to fp32"""
    return STAT_CONV * U32 * mean.abs(), torch.full_like(mean, STAT_CONV * U32)


def row_stats_err(x, eps):
    """(dmean, drstd) [rows] of the two-pass fp32 row statistics"""
    mean, var, _ = ref_row_stats(x, eps)
    dmean = (L_ROW + 1) * U32 * x.double().abs().mean(-1)
    v = var + f32(eps)
    return dmean, rstd_err((L_ROW + 5) * U32 * v + dmean ** 2, v, eps) + 2 * U32


def silu_bound(y, e_y):
    """error of the fp32 SiLU of a y known to within e_y, against silu64(y)"""
    return SILU_LIP * e_y + K_SILU * U32 * (1 + y.abs()) * F.silu(y).abs()


def affine_bound(x, mean_c, rstd_c, dmean_c, drstd_c, gamma, beta, silu, dtype):
    """the per-element bound of the module docstring; every statistic already broadcast against x.  -> (ref, bound, e), float64; e = the part of the bound in
    front of the output rounding"""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    n = (x - mean_c) * rstd_c
    a = (x.abs() + mean_c.abs()) * rstd_c * gamma.abs() + beta.abs()
    e = N_EXPR * U32 * a + dmean_c * rstd_c * gamma.abs() + (n * gamma).abs() * drstd_c
    ref = n * gamma + beta
    if silu:
        e = silu_bound(ref, e)
        ref = F.silu(ref)
    return ref, U_RND[dtype] * (ref.abs() + e) + e + ABS_FLOOR[dtype], e


def gn_bound(x, gamma, beta, groups, eps, silu, dtype, dmean, drstd, stats=None):
    """-> (ref, bound, e) [b][hw][C]; dmean / drstd [b][groups]; `stats` = (mean, rstd) float64 to normalise with (the producer-partial path)"""
    cpg = x.shape[-1] // groups
    if stats is None:
        mean, _, rstd = ref_gn_stats(x, groups, eps)
    else:
        mean, rstd = stats
    return affine_bound(x, per_channel(mean, cpg), per_channel(rstd, cpg), per_channel(dmean, cpg), per_channel(drstd, cpg), gamma, beta, silu, dtype)


def const_bound(v, rstd, gamma, beta, silu, dtype):
    """a group whose every value is v (sums, mean = v and var = 0 exact): the 16-bit kernels compute fl(h + fl(beta - h)) with h = fl(v sc), two roundings
    at the magnitude of h; the fp32 twins fl(0 + beta) = beta.  -> (ref, bound, e), gamma / beta-shaped"""
    gamma, beta = gamma.double(), beta.double()
    e = torch.zeros_like(beta) if dtype == torch.float32 else 2 * U32 * abs(v) * rstd * gamma.abs()
    ref = beta
    if silu:
        e = silu_bound(ref, e)
        ref = F.silu(ref)
    return ref, U_RND[dtype] * (ref.abs() + e) + e + ABS_FLOOR[dtype], e


def ln_bound(x, gamma, beta, eps, dtype):
    mean, _, rstd = ref_row_stats(x, eps)
    dmean, drstd = row_stats_err(x, eps)
    return affine_bound(x, mean[:, None], rstd[:, None], dmean[:, None], drstd[:, None], gamma, beta, 0, dtype)


def scsh_bound(mean, rstd, gamma, beta, cpg):
    """the planes [b][2][C] of gn_finalize_kernel against float64 ones from the same (mean, rstd): sc = fl(rstd32 gamma): 2 u; sh = fl(beta - fl(mean32 sc)):
    mean32, sc (2), the product and the difference"""
    sc = rstd.repeat_interleave(cpg, 1) * gamma.double()
    msc = (mean.repeat_interleave(cpg, 1) * sc).abs()
    return SHORT * torch.stack([2 * U32 * sc.abs(), U32 * (6 * msc + beta.double().abs())], dim=1)


def ln_finalize_err(part, cw, eps):
    """(dmean, drstd) [rows] of the P sequential fp32 updates of ln_finalize_kernel against chan_merge on the same partials.  Per step, with dm / dm2 the
    errors so far: d' = fl(x - mean'): dd = dm + u (|d| + dm);  mean' += fl(d' f'), f' = fl(cw / nt): dm += f dd + 3 u (|d| + dd) f + u |mean|;
    T = d d n f (4 roundings on (|d| + dd)^2 n f, plus the error of d), fl(M2_q + T), fl(m2 + .): one u each"""
    part = part.double()
    n = 0.0
    mean = torch.zeros_like(part[:, 0, 0])
    m2, dm, dm2 = torch.zeros_like(mean), torch.zeros_like(mean), torch.zeros_like(mean)
    for q in range(part.shape[1]):
        nt = n + cw
        f = cw / nt
        d = part[:, q, 0] - mean
        dd = dm + U32 * (d.abs() + dm)
        mean = mean + d * f
        dm = dm + f * dd + 3 * U32 * (d.abs() + dd) * f + U32 * mean.abs()
        t_up = (d.abs() + dd) ** 2 * n * f
        m2 = m2 + part[:, q, 1] + d * d * n * f
        dm2 = dm2 + (2 * d.abs() * dd + dd * dd) * n * f + 4 * U32 * t_up + U32 * (part[:, q, 1] + t_up) + U32 * (m2 + dm2)
        n = nt
    v = m2 / n + f32(eps)
    return dm, rstd_err(dm2 / n + SHORT * 2 * U32 * v, v, eps) + SHORT * 2 * U32


def gemm_ln_bound(x, wp, c_vec, eps, dtype):
    """float64 LayerNorm(x) W'^T + c on the folded 16-bit weights W' and the bound of the issue: one output rounding plus K u rstd sum_k |x_k| |W'_k|.
    -> (ref, bound, e) [m][n]"""
    mean, _, rstd = ref_row_stats(x, eps)
    x64, w64 = x.double(), wp.double()
    ref = ((x64 - mean[:, None]) * rstd[:, None]) @ w64.t() + c_vec.double()
    e = x.shape[1] * U32 * rstd[:, None] * (x64.abs() @ w64.abs().t())
    return ref, U_RND[dtype] * (ref.abs() + e) + e + ABS_FLOOR[dtype], e


def worst(got, ref, bound):
    """worst |got - ref| / bound; a non-finite value counts as inf"""
    r = (got.double() - ref).abs() / bound
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    return float(r.max())


# ---------------------------------------------------------------------------------------------------------------- inputs
IMAGE_SCALES = 16      # rows, and the images of the ratio64 family, are scaled by 1 + i % 16: 1 + i itself leaves fp16 at |mean| / std = 64 once i reaches 200


def image_scales(b, family):
    """image i is scaled by 1 + i (ratio64: 1 + i % 16, the large case has 256 images)"""
    i = torch.arange(b)
    return (1 + (i % IMAGE_SCALES if family == "ratio64" else i)).float()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def norm_params(c, seed, eighths=False):
    """gamma = 1 + 0.1 N, beta = 0.1 N; eighths: beta a non-zero multiple of 1/8 (exact in every io type, half an ulp far above the fp32 roundings of the
    constant cases)"""
    g = _gen(seed)
    gamma, beta = torch.randn(c, generator=g) * 0.1 + 1, torch.randn(c, generator=g) * 0.1
    if eighths:
        beta = (torch.randint(1, 5, (c,), generator=g) * (torch.randint(0, 2, (c,), generator=g) * 2 - 1)).float() / 8
    return gamma, beta


def gn_input(b, hw, c, groups, dtype, family, seed):
    """[b][hw][c] in the io type.  random: N(0.3, 1.5^2) plus a per-channel offset ~ N(0, 2^2), image i scaled by 1 + i: statistics over the wrong channels
    or the wrong image are visibly wrong.  const: 0.5 everywhere.  group_const: random, one group (the one that straddles 2/3 of the width, i.e. the concat
    boundary of 1280 + 640) 0.5 x the image scale.  ratio8 / ratio64: every (image, group) shifted to |mean| / std = 8 / 64, signs alternating"""
    if family == "const":
        return torch.full((b, hw, c), 0.5, dtype=dtype)
    g = _gen(seed)
    cpg = c // groups
    off = 2.0 * torch.randn(c, generator=g)
    x = torch.randn(b, hw, c, generator=g) * 1.5 + off
    scale = image_scales(b, family)[:, None, None]
    if family in ("random", "group_const"):
        x = x + 0.3
        if family == "group_const":
            g0 = const_group(c, groups)
            x[:, :, g0 * cpg:(g0 + 1) * cpg] = 0.5
    else:
        ratio = {"ratio8": 8.0, "ratio64": 64.0}[family]
        v = x.reshape(b, hw, groups, cpg)
        mean = v.mean((1, 3), keepdim=True)
        std = ((v - mean) ** 2).mean((1, 3), keepdim=True).sqrt()
        sign = (1 - 2 * (torch.arange(groups) % 2)).float()[None, None, :, None]
        x = (v - mean + ratio * std * sign).reshape(b, hw, c)
    return (x * scale).to(dtype)


def const_group(c, groups):
    return (2 * c // 3) // (c // groups)


def row_input(rows, c, dtype, family, seed):
    """[rows][c]: N(0, 1.5^2) plus a per-column offset ~ N(0, 2^2), row r scaled by 1 + r % 16.  const_row: rows 0, 2, 7, 12, ... are 0.5 x their scale.
    ratio8 / ratio64: every row shifted to |mean| / std = 8 / 64, signs alternating"""
    g = _gen(seed)
    x = torch.randn(rows, c, generator=g) * 1.5 + 2.0 * torch.randn(c, generator=g)
    if family in ("ratio8", "ratio64"):
        ratio = {"ratio8": 8.0, "ratio64": 64.0}[family]
        mean = x.mean(-1, keepdim=True)
        std = ((x - mean) ** 2).mean(-1, keepdim=True).sqrt()
        x = x - mean + ratio * std * (1 - 2 * (torch.arange(rows) % 2)).float()[:, None]
    elif family == "const_row":
        x[const_rows(rows)] = 0.5
    else:
        assert family == "random"
    return (x * (1 + torch.arange(rows) % IMAGE_SCALES).float()[:, None]).to(dtype)


def const_rows(rows):
    return [r for r in range(rows) if r == 0 or r % 5 == 2]


def lnf_partials(rows, p, cw, family, seed):
    """fp32 [rows][P][2] for ln_finalize.  random: ln_partials of a random fp32 matrix; cross: chunk means 10 k and a spread of 0.1, so that the cross term
    d d n f carries almost all of the variance; chunk_const: chunk P // 2 constant (M2 = 0); all_const: every value 0.5 (rstd = 1 / sqrt(eps))"""
    g = _gen(seed)
    x = torch.randn(rows, p, cw, generator=g)
    if family == "cross":
        x = 0.1 * x + 10.0 * torch.arange(p).float()[None, :, None]
    elif family == "all_const":
        x = torch.full_like(x, 0.5)
    else:
        x = (x * 1.5 + 0.3 + 2.0 * torch.randn(p, cw, generator=g)) * (1 + torch.arange(rows) % IMAGE_SCALES).float()[:, None, None]
        if family == "chunk_const":
            x[:, p // 2] = 0.5
        else:
            assert family == "random"
    return ln_partials(x.reshape(rows, p * cw), p)


# ---------------------------------------------------------------------------------------------------------------- the GPU tests' cases
# GroupNorm, direct: (name, b, hw, c1, c2, groups, family, premise) -- premise: what gn_geometry must say of the case (asserted by both test files)
GN_WIDTHS = [
    ("w320", 2, 72, 320, 0, 32, "random", dict(stats_vpl=1, apply_mode=0)),                 # flat apply, 10 channels per group: groups straddle a vector
    ("w640", 2, 72, 640, 0, 32, "random", dict(stats_vpl=2, apply_mode=0)),                 # flat apply
    ("w256+64", 2, 72, 256, 64, 32, "random", dict(stats_vpl=1, apply_mode=0)),             # flat apply, two sources
    ("w640+320", 2, 72, 640, 320, 32, "random", dict(stats_vpl=2, apply_mode=2)),           # 2 vectors per lane, a group straddles the sources
    ("w1280", 2, 72, 1280, 0, 32, "random", dict(stats_vpl=3, apply_mode=3)),
    ("w1280+640", 2, 72, 1280, 640, 32, "random", dict(stats_vpl=4, apply_mode=4)),         # a group straddles the sources
    ("w1280+1280", 2, 72, 1280, 1280, 32, "random", dict(stats_vpl=5, apply_mode=5)),
    ("w320g8", 2, 72, 320, 0, 8, "random", dict(stats_vpl=1, apply_mode=0)),
    ("w512g64", 2, 72, 512, 0, 64, "random", dict(stats_vpl=1, apply_mode=1, wide_groups=True)),   # the groups > 32 branches of both kernels
]
GN_PIXELS = [(f"c{c}b{b}hw{hw}", b, hw, c, 0, 32, "random",
              dict(chunks=min(64, max(1, hw // 8)), chunks_apply=max(1, hw // 4), **({"empty_stats": list(range(58, 64))} if hw == 520 else {})))
             for c in (320, 1280) for b in (1, 3) for hw in (1, 3, 4, 7, 9, 33, 100, 520)]
GN_BATCH = [
    ("b40hw1024", 40, 1024, 320, 0, 32, "random", dict(chunks=25, chunks_apply=51, empty_apply=[49, 50])),
    ("b1100hw16", 1100, 16, 320, 0, 32, "random", dict(chunks=1, chunks_apply=1)),                    # 1024 / b == 0
    ("b3hw4096", 3, 4096, 320, 0, 32, "random", dict(chunks=64, chunks_apply=682, chain_pixels=16)),
]
GN_FAMILIES = [(f"{fam}{c1}+{c2}", 2, 256, c1, c2, 32, fam, dict(chunks=32, chain_pixels=2))
               for c1, c2 in ((320, 0), (1280, 640)) for fam in ("const", "group_const", "ratio8")]
GN_BIG = ("ratio64b256", 256, 1024, 320, 0, 32, "ratio64", dict(chunks=4, chain_pixels=64))           # the one large case: fp32 chains of 64 pixels
GN_CASES = GN_WIDTHS + GN_PIXELS + GN_BATCH + GN_FAMILIES + [GN_BIG]
# GroupNorm from producer partials: (b, hw, c1, c2, wm1, wm2)
GN_PRE_CASES = [(3, 64, 320, 0, 64, 0), (2, 256, 640, 320, 64, 32), (2, 96, 1280, 1280, 32, 16), (5, 128, 320, 0, 128, 0), (2, 64, 1280, 640, 16, 64)]
GN_PRE_FAMILIES = ["random", "const", "ratio64"]
LN_WIDTHS = [8, 320, 512, 520, 768, 1024, 1280, 1536]          # fp32: up to 1280
LN_ROWS = [1, 3, 4, 5, 130]
LN_FAMILIES = ["random", "const_row", "ratio64"]
LNF_P, LNF_CW, LNF_ROWS = [1, 2, 4, 10, 16], [32, 80, 128], [1, 255, 256, 257, 1000]
LNF_FAMILIES = ["random", "cross", "chunk_const", "all_const"]
GEMM_LN_CASES = [(256, 320, 320), (64, 1280, 3840)]             # (m, c, n) of test_gemm_layernorm_fold: two-slot 64 x 64 tiles; split-K with the LayerNorm in the reduction
EPS_SILU = [(1e-5, 1), (1e-6, 0)]


def check_premise(geo, premise, name):
    for key, want in premise.items():
        assert getattr(geo, key) == want, f"{name}: gn_geometry.{key} = {getattr(geo, key)}, the case was chosen for {want}"


class GnCase:
    """one direct GroupNorm launch: input (CPU, io type), parameters and geometry; references and bounds are computed where the caller puts the tensors"""

    def __init__(self, dtype, name, b, hw, c1, c2, groups, family, premise):
        self.dtype, self.name, self.b, self.hw, self.c1, self.c2, self.groups, self.family = dtype, name, b, hw, c1, c2, groups, family
        self.c = c1 + c2
        self.geo = gn_geometry(b, hw, c1, c2, groups)
        check_premise(self.geo, premise, name)
        self.x = gn_input(b, hw, self.c, groups, dtype, family, seed=b + hw + self.c)
        self.gamma, self.beta = norm_params(self.c, seed=self.c + groups, eighths=family in ("const", "group_const"))
        self.label = f"groupnorm {name} b={b} hw={hw} {c1}+{c2} g={groups} {family} {NAME[dtype]}"

    def stats_err(self, x, eps):
        """(dmean, drstd) of the per-element bound.  ratio8 is held to the bound of the centred group; ratio64 to the conditioned one"""
        if self.dtype == torch.float32:
            return stats_err_double(ref_gn_stats(x, self.groups, eps)[0])
        return gn_stats_err16(x, self.groups, eps, self.geo, centred=self.family == "ratio8")

    def evaluate(self, x, gamma, beta, eps, silu, got=None):
        """-> dict(ref, bound, e, emu, kernel = worst |got - ref| / bound, emulation = the same of the rounded emulation (float64 statistics), arithmetic =
        worst |emulation before its rounding - ref| / e, kernel_order = the same with the statistics summed in fp32 in the kernel's order (16-bit types): a
        prediction of the kernel, not a condition on the bound); tensors on the device of x"""
        dmean, drstd = self.stats_err(x, eps)
        ref, bound, e = gn_bound(x, gamma, beta, self.groups, eps, silu, self.dtype, dmean, drstd)
        emu = emulate_groupnorm(x, gamma, beta, self.groups, eps, silu, self.dtype)
        res = dict(ref=ref, bound=bound, e=e, emu=emu, emulation=worst(emu.to(self.dtype), ref, bound), arithmetic=worst(emu, ref, e))
        if self.dtype != torch.float32:
            emu_k = emulate_groupnorm(x, gamma, beta, self.groups, eps, silu, self.dtype, self.geo)
            res["kernel_order"], res["kernel_order_rounded"] = worst(emu_k, ref, e), worst(emu_k.to(self.dtype), ref, bound)
        if got is not None:
            res["kernel"] = worst(got, ref, bound)
        return res


@functools.lru_cache(maxsize=4)
def gn_case(dtype, name):
    return GnCase(dtype, *next(c for c in GN_CASES if c[0] == name))


class PreCase:
    """one launch_groupnorm_pre call: sources, their hand-made partials, parameters (CPU)"""

    def __init__(self, dtype, b, hw, c1, c2, wm1, wm2, family):
        self.dtype, self.b, self.hw, self.c1, self.c2, self.wm1, self.wm2, self.family, self.groups = dtype, b, hw, c1, c2, wm1, wm2, family, 32
        self.c = c1 + c2
        self.geo = gn_geometry(b, hw, c1, c2)
        x = gn_input(b, hw, self.c, 32, dtype, family, seed=7 + b + hw + self.c)
        self.x1 = x[..., :c1].contiguous()
        self.x2 = x[..., c1:].contiguous() if c2 else None
        self.p1 = gn_partials(self.x1, wm1)
        self.p2 = gn_partials(self.x2, wm2) if c2 else None
        self.gamma, self.beta = norm_params(self.c, seed=self.c + 1, eighths=family == "const")
        self.label = f"groupnorm_pre b={b} hw={hw} {c1}+{c2} wm={wm1}/{wm2} {family} {NAME[dtype]}"

    def evaluate(self, x, p1, p2, gamma, beta, eps, silu):
        """x = cat of the sources.  -> dict(mean, rstd, planes, dmean, drstd, planes_bound, ref, bound, e, emu); the statistics are the float64 finalize of the
        SAME fp32 partials, the emulation rounds them to fp32 and applies x sc + sh"""
        mean, rstd, planes = gn_from_partials(p1, self.wm1, p2, self.wm2, self.b, self.hw, 32, eps, gamma, beta)
        dmean, drstd = stats_err_double(mean)
        ref, bound, e = gn_bound(x, gamma, beta, 32, eps, silu, self.dtype, dmean, drstd, stats=(mean, rstd))
        emu = emulate_groupnorm(x, gamma, beta, 32, eps, silu, self.dtype, stats=(mean, rstd))
        return dict(mean=mean, rstd=rstd, planes=planes, dmean=dmean, drstd=drstd, planes_bound=scsh_bound(mean, rstd, gamma, beta, self.c // 32),
                    ref=ref, bound=bound, e=e, emu=emu, emulation=worst(emu.to(self.dtype), ref, bound), arithmetic=worst(emu, ref, e))


@functools.lru_cache(maxsize=4)
def pre_case(dtype, idx, family):
    return PreCase(dtype, *GN_PRE_CASES[idx], family)


def ln_params(c):
    return norm_params(c, seed=3 * c + 1)


def gemm_ln_inputs(m, c, n, dtype):
    """rows at |mean| / std = 8, an fp32 Linear (w, bias) and LayerNorm parameters; (x, w, gamma, beta, bias)"""
    g = _gen(m + c + n)
    x = row_input(m, c, dtype, "ratio8", seed=m + c)
    return x, torch.randn(n, c, generator=g) * c ** -0.5, 1.0 + 0.3 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g), torch.randn(n, generator=g)


def fold_ref(w, gamma, beta, bias, dtype):
    """what etainv_op_ln_fold leaves (plain packing): W' = (W gamma) rounded to the io type, s = row sums of W', c = W beta + bias; float64 s and c"""
    wp = (w.float() * gamma.float()).to(dtype)
    return wp, wp.double().sum(1), w.double() @ beta.double() + bias.double()
